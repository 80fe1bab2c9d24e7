"""CPU: the floor estimator's rule.  tests/floor_ref.py (the float64 restatement tests/test_gpu_floor.py holds csrc/floor.hip to)
against hand-computable cases, the host logic of rohm_amd/floor.py (triples, the camera pose, the refusals), and planted
floors.  The entry points that launch kernels have no CPU path: only their refusal is checked here.

Bars.  Noise-free planted floor: 1e-9 (rad, m) -- the track holds float32 points that lie on the planted plane exactly
(`floor_ref.planted_track`), so only float64 rounding is left.  Noisy planted floor (Gaussian, sigma = 5 mm along the normal,
one draw per contact): the first-order standard errors of a least-squares plane through `support` points are sigma /
(extent sqrt(support)) for the normal's angle (extent = the spread in the second direction, the weaker lever) and sigma /
sqrt(support) for the height at the contacts' centroid; the bars are 5 of those, derived in the test from the estimate's own
support and extent.  The measured maxima go to profiles/floor_parity.json."""
import json

import numpy as np
import pytest
import torch

import floor_ref as FR
from rohm_amd import floor as FL

SIGMA, record = FR.SIGMA, FR.record


# ---- 1. hand-computable planes ---------------------------------------------------------------------------------------------
SQUARE = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], np.float32)
TRIPLE = np.array([[0, 1, 2]], np.int32)


def _above(z, n=5):
    return np.array([[0.2 * k, 0.5, z] for k in range(n)], np.float32)


def test_four_coplanar_toes_with_a_body_above_give_the_plane():
    planes, scores, best = FR.hypotheses(SQUARE, _above(1.0), TRIPLE, tau=0.03, under_tol=0.08)
    assert np.array_equal(planes, [[0.0, 0.0, 1.0, 0.0]]) and scores.tolist() == [[4, 4, 0]] and best == 0
    # a point off the plane by more than tau does not support it; a joint more than under_tol below counts against it
    pts = np.concatenate([SQUARE, [[0.5, 0.5, 0.05]]]).astype(np.float32)
    jts = np.concatenate([_above(1.0), [[0.5, 0.5, -0.2]], [[0.5, 0.5, -0.05]]]).astype(np.float32)
    planes, scores, best = FR.hypotheses(pts, jts, TRIPLE)
    assert scores.tolist() == [[3, 4, 1]]


def test_the_plane_turns_towards_the_body_and_a_tie_keeps_it():
    jts = np.concatenate([_above(-1.0), _above(1.0, 1)])
    planes, scores, best = FR.hypotheses(SQUARE, jts, TRIPLE)
    assert np.array_equal(planes[0, :3], [0.0, 0.0, -1.0]) and planes[0, 3] == 0.0 and scores.tolist() == [[3, 4, 1]]
    planes, scores, best = FR.hypotheses(SQUARE, np.concatenate([_above(-1.0, 2), _above(1.0, 2)]), TRIPLE)
    assert np.array_equal(planes[0], [0.0, 0.0, 1.0, 0.0]) and scores.tolist() == [[2, 4, 2]]


def test_a_degenerate_triple_gives_the_sentinel():
    pts = np.concatenate([SQUARE, [[2, 0, 0]], [[np.nan, 0, 0]]]).astype(np.float32)
    tr = np.array([[0, 0, 1], [0, 1, 4], [0, 1, 5], [0, 1, 2]], np.int32)            # repeated, collinear, NaN, fine
    planes, scores, best = FR.hypotheses(pts, _above(1.0), tr)
    assert np.isnan(planes[:3]).all() and scores[:3].tolist() == [[FR.INT64_MIN, 0, 0]] * 3
    assert np.array_equal(planes[3], [0.0, 0.0, 1.0, 0.0]) and scores[3].tolist() == [5, 5, 0] and best == 3     # the NaN point supports nothing
    assert FR.hypotheses(pts, _above(1.0), tr[:3])[2] == -1
    # a NaN joint is in no count
    jts = np.concatenate([_above(1.0), [[np.nan, 0, -1.0]]]).astype(np.float32)
    assert FR.hypotheses(SQUARE, jts, TRIPLE)[1].tolist() == [[4, 4, 0]]


# ---- 2. the candidate rule, one case per clause ---------------------------------------------------------------------------------
def _still(N=6):
    j = np.zeros((N, 22, 3), np.float32)
    j[:, 10] = (0.1, 0.2, 3.0)
    j[:, 11] = (-0.1, 0.2, 3.0)
    kp = np.ones((N, 22, 3), np.float32)
    return j, np.arange(N) / 30.0, kp


def test_candidate_rule():
    j, t, kp = _still()
    all_valid = np.arange(6)
    want = np.ones((6, 2), np.uint8)
    want[5] = 0                                                                    # the last frame has no successor
    assert np.array_equal(FR.candidates(j, t, all_valid, kp, max_gap=0.05), want)
    assert np.array_equal(FR.candidates(j, t, all_valid, None, max_gap=0.05), want)
    # an invalid frame: frame 2 is no candidate, and frame 1's successor is frame 3, two intervals away
    flags = FR.candidates(j, t, np.array([0, 1, 3, 4, 5]), kp, max_gap=0.05)
    assert flags[:, 0].tolist() == [1, 0, 0, 1, 1, 0]
    assert FR.candidates(j, t, np.array([0, 1, 3, 4, 5]), kp, max_gap=0.07)[:, 0].tolist() == [1, 1, 0, 1, 1, 0]
    # a next frame beyond max_gap
    t2 = t.copy()
    t2[3:] += 1.0
    assert FR.candidates(j, t2, all_valid, kp, max_gap=0.05)[:, 0].tolist() == [1, 1, 0, 1, 1, 0]
    # a fast toe: 1 cm in 1/30 s is 0.3 m/s; 2 mm is 0.06 m/s
    j2 = j.copy()
    j2[3:, 10, 0] += 0.01
    j2[4:, 11, 2] += 0.002
    flags = FR.candidates(j2, t, all_valid, kp, max_gap=0.05)
    assert flags[:, 0].tolist() == [1, 1, 0, 1, 1, 0] and flags[:, 1].tolist() == [1, 1, 1, 1, 1, 0]
    # low confidence, at the frame itself
    kp2 = kp.copy()
    kp2[1, 11, 2] = 0.1
    kp2[2, 11, 2] = 0.2                                                            # not above conf_min
    flags = FR.candidates(j, t, all_valid, kp2, conf_min=0.2, max_gap=0.05)
    assert flags[:, 0].tolist() == [1, 1, 1, 1, 1, 0] and flags[:, 1].tolist() == [1, 0, 0, 1, 1, 0]
    # a NaN position spoils the pair before it and the pair after it; a NaN confidence or time likewise
    j3 = j.copy()
    j3[2, 10, 1] = np.nan
    assert FR.candidates(j3, t, all_valid, kp, max_gap=0.05)[:, 0].tolist() == [1, 0, 0, 1, 1, 0]
    kp3 = kp.copy()
    kp3[0, 10, 2] = np.nan
    assert FR.candidates(j, t, all_valid, kp3, max_gap=0.05)[:, 0].tolist() == [0, 1, 1, 1, 1, 0]
    t3 = t.copy()
    t3[4] = np.nan
    assert FR.candidates(j, t3, all_valid, kp, max_gap=0.05)[:, 0].tolist() == [1, 1, 1, 0, 0, 0]
    assert FR.candidate_points(j, want).shape == (10, 3) and np.array_equal(FR.candidate_points(j, want)[:2], j[0, 10:12])


# ---- 3. the camera pose ---------------------------------------------------------------------------------------------------------------
def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


@pytest.mark.parametrize('up_axis', ('z', 'y'))
@pytest.mark.parametrize('pose', (FL.cam2world_from_plane, FR.pose), ids=('module', 'restatement'))
def test_cam2world(pose, up_axis):
    e = np.eye(3)[FL.UP_AXIS[up_axis]]
    g = np.random.Generator(np.random.PCG64(3))
    normals = [_unit(g.standard_normal(3)) for _ in range(8)] + [-e, e, np.array([1.0, 0.0, 0.0]), np.array([-1.0, 0.0, 0.0])]
    for n in normals:
        d = float(g.uniform(-3, 3))
        M = pose(n, d, up_axis)
        R = M[:3, :3]
        assert np.abs(R @ n - e).max() < 1e-12 and abs(np.linalg.det(R) - 1.0) < 1e-12 and np.abs(R @ R.T - np.eye(3)).max() < 1e-12
        assert np.array_equal(M[3], [0, 0, 0, 1])
        p = g.uniform(-3, 3, size=(20, 3))
        up = (p @ R.T + M[:3, 3])[:, FL.UP_AXIS[up_axis]]
        assert np.abs(up - (p @ n + d)).max() < 1e-12
    assert np.array_equal(pose(e, 0.0, up_axis), np.eye(4))                     # the minimal rotation of nothing
    n_g, d_g = FL.plane_of_calibration(FL.cam2world_from_plane(normals[0], 0.7, up_axis), up_axis, floor_height=0.2)
    assert np.abs(n_g - normals[0]).max() < 1e-12 and abs(d_g - 0.5) < 1e-12
    with pytest.raises(ValueError, match='up_axis'):
        FL.cam2world_from_plane(e, 0.0, 'x')


# ---- 4. triples, seeds ------------------------------------------------------------------------------------------------------------------
def test_the_same_seed_gives_the_same_triples():
    a, b, c = FL.draw_triples(100, 64, 7), FL.draw_triples(100, 64, 7), FL.draw_triples(100, 64, 8)
    assert a.dtype == np.int32 and a.shape == (64, 3) and np.array_equal(a, b) and not np.array_equal(a, c)
    assert a.min() >= 0 and a.max() < 100
    assert np.array_equal(a, np.random.Generator(np.random.PCG64(7)).integers(0, 100, size=(64, 3)))


CLEAN = {}


def clean_track():
    if not CLEAN:
        CLEAN['j'], CLEAN['on'] = FR.planted_track(stances=200, sigma=0.0, seed=1)
        CLEAN['j'].setflags(write=False)
    return CLEAN['j'], CLEAN['on']


def test_planted_floor_noise_free_and_seeds():
    """A tilted plane with 20 % of the contacts on a step 0.4 m higher: angle and offset within 1e-9, whatever the seed."""
    j, on = clean_track()
    n, d = FR.planted_plane()
    ests = [FR.estimate_floor(j, hypotheses=256, seed=s) for s in (0, 1, 2)]
    for est in ests:
        angle, off = FR.plane_errors(est)
        print(f'noise-free: angle {angle:.3e} rad, centroid off the plane {off:.3e} m, offset {abs(est.offset - d):.3e} m (bar 1e-9)')
        record('cpu', 'noise_free_angle_rad', angle)
        record('cpu', 'noise_free_offset_m', abs(est.offset - d))
        assert angle <= 1e-9 and off <= 1e-9 and abs(est.offset - d) <= 1e-9
        assert est.candidates == 2 * len(on) and est.support == 2 * int(on.sum()) and est.under == 0 and est.rms < 1e-9
        assert est.floor_height == 0.0 and est.up_axis == 'z' and 0.2 < est.extent < 0.7
        assert abs(est.tilt_deg - np.degrees(np.arccos(-n[1]))) < 1e-6
    assert ests[0].hypothesis != ests[1].hypothesis or ests[0].hypothesis != ests[2].hypothesis
    assert np.abs(ests[0].normal - ests[1].normal).max() < 1e-12 and abs(ests[0].offset - ests[2].offset) < 1e-12
    same = FR.estimate_floor(j, hypotheses=256, seed=0)
    assert np.array_equal(same.normal, ests[0].normal) and same.offset == ests[0].offset and same.hypothesis == ests[0].hypothesis
    est = FR.estimate_floor(j, hypotheses=256, up_axis='y', toe_height=0.02)
    assert est.floor_height == -0.02 and np.abs(est.cam2world[:3, :3] @ est.normal - [0, 1, 0]).max() < 1e-12


@pytest.mark.parametrize('seed', (0, 1, 2, 3))
def test_planted_floor_noisy(seed):
    j, on = FR.planted_track(stances=200, sigma=SIGMA, seed=10 + seed)
    est = FR.estimate_floor(j, hypotheses=512, seed=seed)
    angle, off = FR.plane_errors(est)
    bar_angle, bar_off = 5 * SIGMA / (est.extent * np.sqrt(est.support)), 5 * SIGMA / np.sqrt(est.support)
    print(f'seed {seed}: support {est.support} of {est.candidates}, extent {est.extent:.3f} m, rms {est.rms * 1e3:.2f} mm; '
          f'angle {angle:.3e} rad (bar {bar_angle:.3e}), height at the centroid {off:.3e} m (bar {bar_off:.3e})')
    record('cpu', 'noisy_angle_over_bar', angle / bar_angle)
    record('cpu', 'noisy_offset_over_bar', off / bar_off)
    assert est.support >= 2 * int(on.sum()) - 2 and est.support <= 2 * int(on.sum())
    assert 0.5 * SIGMA < est.rms < 1.5 * SIGMA
    assert angle <= bar_angle and off <= bar_off


# ---- 5. the refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_and_force():
    j, on = clean_track()
    with pytest.raises(ValueError, match=r'only 24 resting toe positions.*min_candidates=30'):
        FR.estimate_floor(j[:24], hypotheses=64)
    assert FR.estimate_floor(j[:24], hypotheses=64, strict=False).candidates == 24
    with pytest.raises(ValueError, match='a plane needs 3'):
        FR.estimate_floor(j[:2], hypotheses=64, strict=False)
    # a fifth of the stances stand on the step: the support is about 0.8, below min_support=0.9
    with pytest.raises(ValueError, match=r'min_support=0.9'):
        FR.estimate_floor(j, hypotheses=64, min_support=0.9)
    assert FR.estimate_floor(j, hypotheses=64, min_support=0.9, strict=False).support == 2 * int(on.sum())
    # contacts on one line: the person walks along x only, the two feet 4 mm apart
    line = np.array(j)
    line[:, :, 1] = -1.0                                                          # the body is up the camera's -y
    line[:, 10, 1], line[:, 11, 1] = 0.002, -0.002
    line[:, :, 2] = 0.25 * line[:, :, 0] + 3.0
    with pytest.raises(ValueError, match=r'extend 0\.00\d m.*min_extent=0\.1'):
        FR.estimate_floor(line, hypotheses=64)
    est = FR.estimate_floor(line, hypotheses=64, strict=False)
    assert est.extent < 0.01 and est.support == est.candidates
    with pytest.raises(ValueError, match='up_axis'):
        FR.estimate_floor(j, up_axis='x')


def test_compare_planes():
    j, on = clean_track()
    est = FR.estimate_floor(j, hypotheses=64)
    angle, diff = FL.compare_planes(est, est.cam2world, 'z', est.floor_height)
    assert angle < 1e-6 and abs(diff) < 1e-12
    assert FL.compare_planes(est, est.cam2world, 'z')[1] is None
    M = est.cam2world.copy()
    M[2, 3] += 0.1                                                                # the world 10 cm higher: the floor is 10 cm lower
    assert abs(FL.compare_planes(est, M, 'z', 0.0)[1] - 0.1) < 1e-12
    tilt = FL.cam2world_from_plane(_unit(est.normal + np.array([0.0, 0.0, 0.02])), est.offset)
    assert 0.3 < FL.compare_planes(est, tilt, 'z', 0.0)[0] < 0.7
    d = est.as_dict()
    assert set(d) == set(FL.ESTIMATE_FIELDS) and json.loads(json.dumps(d))['support'] == est.support and len(est.lines()) == 11


# ---- 6. no CPU path ----------------------------------------------------------------------------------------------------------------------------
def test_cpu_tensors_are_refused():
    from rohm_amd._lib import RohmHipError
    j = torch.zeros(4, 22, 3)
    with pytest.raises(RohmHipError, match='no CPU fallback'):
        FL.estimate_floor(j)
    with pytest.raises(RohmHipError, match='no CPU fallback'):
        FL.check_floor(j, np.eye(4), 'z')
    with pytest.raises(RohmHipError, match='no CPU fallback'):
        FL.floor_candidates(j, torch.zeros(4, dtype=torch.float64), torch.arange(4, dtype=torch.int32))
    with pytest.raises(RohmHipError, match='no CPU fallback'):
        FL.floor_hypotheses(j[0], j[0], torch.zeros(1, 3, dtype=torch.int32))
    with pytest.raises(RohmHipError, match='no CPU fallback'):
        FL.floor_moments(j[0], torch.zeros(4, dtype=torch.float64), torch.zeros(3, dtype=torch.float64))
    with pytest.raises(TypeError):
        FL.estimate_floor(np.zeros((4, 22, 3), np.float32))
    with pytest.raises(SystemExit):
        FL.main(['--track', 'nowhere.npz'])
