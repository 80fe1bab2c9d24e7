"""GPU: the floor of an uncalibrated track -- `rohm_floor_candidates`, `rohm_floor_hypotheses`, `rohm_floor_moments`
(csrc/floor.hip) against their float64 restatement (tests/floor_ref.py, held to hand-computable cases in
tests/test_floor_ref.py), `estimate_floor` / `check_floor` on planted floors, and `python -m rohm_amd.floor` end to end with
the synthetic body layer.

Kernel and restatement are both float64 on the same float32 inputs and differ by operation order and fma contraction only, a
few 1e-16 of the distances compared.  Bars: flags, counts, scores and `best` equal as integers wherever no compared distance
lies within `MARGIN` = 1e-9 m of its threshold -- the restatement says which hypotheses those are, at most 1 % of K may be left
out, and the seeds below leave out none --; speeds and confidences are kept 1e-6 away from theirs, asserted on the host; real
outputs within 1e-12 of the output's largest magnitude, the bar of the project's other float64 kernels.  Planted floors: the
bars of tests/test_floor_ref.py.  The measured maxima go to profiles/floor_parity.json."""
import json
import os

import numpy as np
import pytest
import torch

import floor_ref as FR
import video_tree as VT
from rohm_amd.utils import synth

SIGMA, record = FR.SIGMA, FR.record
pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BAR = 1e-12
MARGIN = 1e-9
TAU, UNDER = 0.03, 0.08


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)            # a copy: the shared inputs are read-only


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def make_hyp_inputs(P, N, K, seed):
    """P contacts within 1 cm of the plane z = 0.1 x + 3 (every fifth one 5 .. 40 cm off it), N frames of 22 joints mostly on
    its -z side (the normal of a triple points either way: both the turned and the kept case occur), K random triples.  Where
    the sizes allow: triple 1 repeats an index, triple 2 is collinear (the last three points), point 5 and joint 7 are NaN."""
    g = np.random.Generator(np.random.PCG64(seed))
    xy = g.uniform(-1.0, 1.0, size=(P, 2))
    off = np.where(np.arange(P) % 5 == 4, g.uniform(0.05, 0.4, size=P), g.normal(0.0, 0.01, size=P))
    pts = np.concatenate([xy, (0.1 * xy[:, 0] + 3.0 - off)[:, None]], axis=1)
    jxy = g.uniform(-1.0, 1.0, size=(N * 22, 2))
    h = np.where(g.uniform(size=N * 22) < 0.9, g.uniform(0.0, 1.7, size=N * 22), g.uniform(-0.3, 0.0, size=N * 22))
    jts = np.concatenate([jxy, (0.1 * jxy[:, 0] + 3.0 - h)[:, None]], axis=1)
    tr = g.integers(0, P, size=(K, 3)).astype(np.int32)
    if P >= 65:
        pts[P - 3:] = [[0.0, 0.0, 3.0], [0.5, 0.0, 3.0], [1.0, 0.0, 3.0]]
        pts[5] = np.nan
        if K >= 3:
            tr[2] = (P - 3, P - 2, P - 1)
        if K >= 4:
            tr[3, 0] = 5
    if K >= 2:
        tr[1] = (tr[1, 0], tr[1, 0], tr[1, 2])
    if N >= 2:
        jts[7] = np.nan
    return pts.astype(np.float32), jts.astype(np.float32), tr


HYP_CASES = ((3, 1, 1, 0), (3, 2, 1, 1), (4, 2, 63, 2), (65, 50, 64, 3), (1031, 1031, 65, 4), (1031, 50, 1000, 5), (65, 1031, 1000, 6))
HYP = {}


def hyp_inputs_and_ref(case):
    """The inputs of a case with the restatement's planes, scores, best and margins, computed once and shared."""
    if case not in HYP:
        pts, jts, tr = make_hyp_inputs(*case)
        HYP[case] = (pts, jts, tr) + FR.hypotheses(pts, jts, tr, TAU, UNDER, margins=True)
        for a in HYP[case]:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return HYP[case]


def run_hypotheses(pts, jts, tr, tau=TAU, under_tol=UNDER):
    from rohm_amd.floor import floor_hypotheses
    planes, scores, best = floor_hypotheses(_dev(pts), _dev(jts), _dev(tr), tau, under_tol)
    return planes.cpu().numpy(), scores.cpu().numpy(), int(best.cpu()[0])


# ---- 1. hypotheses against the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize('case', HYP_CASES, ids=lambda c: 'P%d_N%d_K%d' % c[:3])
def test_hypotheses_match_the_restatement(case):
    P, N, K, _ = case
    pts, jts, tr, planes_want, scores_want, best_want, margin = hyp_inputs_and_ref(case)
    left_out = margin < MARGIN
    assert left_out.sum() <= K // 100, (left_out.sum(), K)
    assert not left_out.any(), 'the seeds were chosen so that no hypothesis has a distance within MARGIN of a threshold'
    live = scores_want[:, 0] != FR.INT64_MIN
    if K >= 63:
        raw = FR.triple_planes(pts, tr)[0]
        turned = (np.sign(raw[live, 2]) != np.sign(planes_want[live, 2]))
        assert 0 < turned.sum() < live.sum()                                        # both cases
        assert (~live).sum() >= 1 and (scores_want[live, 2] > 0).any()
    if P >= 65 and K >= 4:
        assert not live[1] and not live[2] and not live[3] and (tr[live] != 5).all()           # repeated, collinear, the NaN point
    planes, scores, best = run_hypotheses(pts, jts, tr)
    assert planes.dtype == np.float64 and scores.dtype == np.int64 and planes.shape == (K, 4) and scores.shape == (K, 3)
    assert np.array_equal(scores[~left_out], scores_want[~left_out]), np.flatnonzero((scores != scores_want).any(axis=1))[:10]
    assert best == best_want
    assert np.array_equal(np.isnan(planes), np.isnan(planes_want)) and np.isnan(planes[~live]).all()
    if live.any():
        rel = np.abs(planes[live] - planes_want[live]).max() / np.abs(planes_want[live]).max()
        print(f'P={P} N={N} K={K}: planes max |kernel - restatement| / max |plane| = {rel:.3e} (bar {BAR:.0e}); best {best}')
        record('gpu', 'hypotheses_planes_max_rel', rel)
        assert rel <= BAR


def test_hypotheses_turned_and_kept():
    """K = 1: the same three points in both orders: one plane is turned over, the other kept, and they are the same plane."""
    pts, jts, tr = make_hyp_inputs(3, 2, 1, 1)
    out = []
    for order in ((0, 1, 2), (0, 2, 1)):
        t = np.array([order], np.int32)
        planes, scores, best = run_hypotheses(pts, jts, t)
        pw, sw, bw = FR.hypotheses(pts, jts, t, TAU, UNDER)
        raw = FR.triple_planes(pts, t)[0]
        assert np.array_equal(scores, sw) and best == bw == 0 and np.abs(planes - pw).max() <= BAR * np.abs(pw).max()
        out.append((planes[0], bool(np.sign(raw[0, 2]) != np.sign(pw[0, 2]))))
    assert out[0][1] != out[1][1] and np.abs(out[0][0] - out[1][0]).max() < 1e-12


def test_all_degenerate_gives_minus_one_and_k0_is_no_launch():
    from rohm_amd.floor import floor_hypotheses
    pts, jts, _ = make_hyp_inputs(65, 2, 3, 3)
    tr = np.array([[0, 0, 1], [64, 63, 62], [5, 1, 2]], np.int32)
    planes, scores, best = run_hypotheses(pts, jts, tr)
    assert best == -1 and np.isnan(planes).all() and scores.tolist() == [[FR.INT64_MIN, 0, 0]] * 3
    planes, scores, best = floor_hypotheses(_dev(pts), _dev(jts), torch.empty(0, 3, dtype=torch.int32, device=DEV))
    assert tuple(planes.shape) == (0, 4) and int(best.cpu()[0]) == -1
    # no joints at all: nothing is under any plane
    planes, scores, best = run_hypotheses(pts, jts[:0], np.array([[0, 1, 2]], np.int32))
    want = FR.hypotheses(pts, jts[:0], np.array([[0, 1, 2]], np.int32), TAU, UNDER)
    assert np.array_equal(scores, want[1]) and scores[0, 2] == 0


# ---- 2. candidates -----------------------------------------------------------------------------------------------------------------
def make_track(N, seed):
    """Toes that rest (0.02 .. 0.08 m/s) or move (0.15 .. 0.6 m/s) at random, 15 % of the frames without a fit, a frame time
    that slips by 2 s in the middle, confidences 1e-3 away from 0.2 at least, one NaN position and one NaN confidence."""
    g = np.random.Generator(np.random.PCG64(seed))
    j = g.uniform(-0.5, 0.5, size=(N, 22, 3))
    speed = np.where(g.uniform(size=(N, 2)) < 0.5, g.uniform(0.02, 0.08, size=(N, 2)), g.uniform(0.15, 0.6, size=(N, 2)))
    step = g.standard_normal(size=(N, 2, 3))
    step = step / np.linalg.norm(step, axis=-1, keepdims=True) * (speed / 30.0)[..., None]
    j[:, 10:12] = g.uniform(-0.3, 0.3, size=(1, 2, 3)) + np.cumsum(step, axis=0) + (0.0, 0.0, 3.0)
    t = np.arange(N) / 30.0
    t[N // 2:] += 2.0 if N > 3 else 0.0
    valid = g.uniform(size=N) > 0.15
    valid[:2] = True
    conf = g.uniform(0.0, 1.0, size=(N, 22))
    conf = np.where(np.abs(conf - 0.2) < 1e-3, 0.25, conf)
    kp = np.concatenate([g.uniform(0, 1000, size=(N, 22, 2)), conf[..., None]], axis=-1)
    if N >= 50:
        j[20, 10, 1] = np.nan
        kp[30, 11, 2] = np.nan
    return j.astype(np.float32), t, valid, kp.astype(np.float32)


def run_candidates(j, t, vi, kp, conf_min=0.2, v_max=0.10, max_gap=0.05):
    from rohm_amd.floor import floor_candidates
    return floor_candidates(_dev(j), _dev(t), _dev(vi.astype(np.int32)), _dev(kp), conf_min, v_max, max_gap).cpu().numpy()


@pytest.mark.parametrize('N', (1, 2, 50, 1031))
def test_candidates_match_the_restatement(N):
    j, t, valid, kp = make_track(N, 200 + N)
    vi = np.flatnonzero(valid)
    if len(vi) > 1:
        _, dt, speed = FR.candidate_terms(j, t, vi)
        with np.errstate(invalid='ignore'):
            assert np.nanmin(np.abs(speed - 0.10)) >= 1e-6 and np.abs(dt - 0.05).min() >= 1e-6
        conf = kp[:, 10:12, 2].astype(np.float64)
        assert np.nanmin(np.abs(conf - float(np.float32(0.2)))) >= 1e-6
    for keypoints in (kp, None):
        want = FR.candidates(j, t, vi, keypoints, 0.2, 0.10, 0.05)
        got = run_candidates(j, t, vi, keypoints)
        assert got.dtype == np.uint8 and got.shape == (N, 2) and np.array_equal(got, want)
        assert np.array_equal(run_candidates(j, t, vi, keypoints), got)              # the same input, the same bits
        if N >= 50:
            assert 0.1 * N < want.sum() < 1.2 * N and not want[~valid].any()
            if keypoints is None:
                assert not want[19, 0] and not want[20, 0]                            # the NaN position spoils both of its pairs
            else:
                assert not want[30, 1]
            gap_frame = vi[vi < N // 2][-1]
            assert not want[gap_frame].any()                                          # its successor is 2 s away
    # nothing valid: every flag is written, as 0
    assert not run_candidates(j, t, vi[:0], kp).any() and not run_candidates(j, t, vi[:1], kp).any()


# ---- 3. moments ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P', (1, 3, 65, 1031))
def test_moments_match_the_restatement(P):
    from rohm_amd.floor import floor_moments
    pts = make_hyp_inputs(max(P, 3), 1, 1, 40 + P)[0][:P]
    plane = np.array([0.1, 0.0, -1.0, 3.0]) / np.sqrt(1.01)
    origin = np.array([0.1, -0.2, 3.0])
    with np.errstate(invalid='ignore'):
        r = pts.astype(np.float64) @ plane[:3] + plane[3]
        assert np.nanmin(np.abs(np.abs(r) - TAU)) >= MARGIN
    want = FR.moments(pts, plane, origin, TAU)
    got = floor_moments(_dev(pts), _dev(plane), _dev(origin), TAU)
    again = floor_moments(_dev(pts), _dev(plane), _dev(origin), TAU)
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))
    got = got.cpu().numpy()
    assert got.dtype == np.float64 and got.shape == (11,) and got[0] == want[0]
    if P >= 65:
        assert 0.5 * P < want[0] < P
    rel = np.abs(got - want).max() / max(np.abs(want).max(), 1e-300)
    print(f'P={P}: moments max |kernel - restatement| / max |moment| = {rel:.3e} (bar {BAR:.0e}), {int(want[0])} inliers')
    record('gpu', 'moments_max_rel', rel)
    assert rel <= BAR
    assert not floor_moments(_dev(pts[:0]), _dev(plane), _dev(origin), TAU).cpu().numpy().any()


# ---- 4. the same input twice ------------------------------------------------------------------------------------------------------------
def test_hypotheses_same_input_same_bits():
    pts, jts, tr = hyp_inputs_and_ref(HYP_CASES[5])[:3]
    a, b = run_hypotheses(pts, jts, tr), run_hypotheses(pts, jts, tr)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]


# ---- 5. bad arguments -----------------------------------------------------------------------------------------------------------------------
def test_kernels_refuse_bad_arguments():
    from rohm_amd import _lib
    from rohm_amd.floor import floor_candidates, floor_hypotheses
    lib, stream = _lib.lib(), _lib.stream_ptr(torch.device(DEV))
    pts, jts, tr = (_dev(a) for a in make_hyp_inputs(65, 2, 4, 9))
    planes, scores = torch.empty(4, 4, device=DEV, dtype=torch.float64), torch.empty(4, 3, device=DEV, dtype=torch.int64)
    best = torch.empty(1, device=DEV, dtype=torch.int32)

    def hyp(P=65, NJ=44, K=4, points=pts.data_ptr(), triples=tr.data_ptr(), tau=TAU):
        return lib.rohm_floor_hypotheses(points, P, jts.data_ptr(), NJ, triples, K, tau, UNDER, planes.data_ptr(), scores.data_ptr(),
                                         best.data_ptr(), stream)
    assert hyp() == 0 and hyp(K=0, points=None) == 0
    assert hyp(P=-1) == -1 and b'negative size' in lib.rohm_last_error()
    assert hyp(points=None) == -1 and b'null' in lib.rohm_last_error()
    assert hyp(P=2) == -1 and b'needs 3 points' in lib.rohm_last_error()
    assert hyp(tau=float('nan')) == -1 and b'tau' in lib.rohm_last_error()
    bad = tr.clone()
    bad[2, 1] = 65
    assert hyp(triples=bad.data_ptr()) == -1 and b'triples[2][1] = 65 is outside [0, 65)' in lib.rohm_last_error()
    bad[2, 1] = -1
    assert hyp(triples=bad.data_ptr()) == -1 and b'triples[2][1] = -1' in lib.rohm_last_error()
    with pytest.raises(_lib.RohmHipError, match=r'outside \[0, 65\)'):
        floor_hypotheses(pts, jts, (tr + 62).contiguous())

    j, t, valid, kp = make_track(50, 1)
    jd, td, vd, flags = _dev(j), _dev(t), _dev(np.flatnonzero(valid).astype(np.int32)), torch.empty(50, 2, device=DEV, dtype=torch.uint8)

    def cand(N=50, Nv=int(valid.sum()), joints=jd.data_ptr(), v_max=0.1, max_gap=0.05):
        return lib.rohm_floor_candidates(joints, td.data_ptr(), vd.data_ptr(), None, N, Nv, 0.2, v_max, max_gap, flags.data_ptr(), stream)
    assert cand() == 0 and cand(N=0, Nv=0, joints=None) == 0
    assert cand(N=-1) == -1 and b'Nv <= N' in lib.rohm_last_error()
    assert cand(Nv=51) == -1 and b'Nv <= N' in lib.rohm_last_error()
    assert cand(joints=None) == -1 and b'null' in lib.rohm_last_error()
    assert cand(v_max=0.0) == -1 and b'v_max' in lib.rohm_last_error()
    assert cand(max_gap=float('nan')) == -1 and b'max_gap' in lib.rohm_last_error()
    # an index outside the track marks nothing and reads nothing
    vi = np.flatnonzero(valid).astype(np.int32)
    vi_bad = vi.copy()
    vi_bad[3] = 50
    got = floor_candidates(jd, td, _dev(vi_bad)).cpu().numpy()
    want = FR.candidates(j, t, vi, None)
    want[vi[2]] = want[vi[3]] = 0
    assert np.array_equal(got, want)
    with pytest.raises(ValueError, match=r'\[N, 22, 3\]'):
        floor_candidates(jd[:, :21], td, vd)

    plane, origin, out = _dev(np.array([0.0, 0.0, 1.0, 0.0])), _dev(np.zeros(3)), torch.empty(11, device=DEV, dtype=torch.float64)

    def mom(P=65, points=pts.data_ptr(), tau=TAU):
        return lib.rohm_floor_moments(points, P, plane.data_ptr(), origin.data_ptr(), tau, out.data_ptr(), stream)
    assert mom() == 0 and mom(P=0, points=None) == 0
    assert mom(P=-1) == -1 and b'P must be' in lib.rohm_last_error()
    assert mom(points=None) == -1 and b'null' in lib.rohm_last_error()
    assert mom(tau=-1.0) == -1 and b'tau' in lib.rohm_last_error()
    torch.cuda.synchronize()


# ---- 6. planted floors ------------------------------------------------------------------------------------------------------------------------
PLANTED = {}


def planted():
    if not PLANTED:
        PLANTED['j'], PLANTED['on'] = FR.planted_track(stances=200, sigma=SIGMA, seed=10)
        PLANTED['j'].setflags(write=False)
        PLANTED['ref'] = {up: FR.estimate_floor(PLANTED['j'], hypotheses=512, seed=0, up_axis=up) for up in ('z', 'y')}
    return PLANTED['j'], PLANTED['on'], PLANTED['ref']


def bars(est):
    return 5 * SIGMA / (est.extent * np.sqrt(est.support)), 5 * SIGMA / np.sqrt(est.support)


@pytest.mark.parametrize('up_axis', ('z', 'y'))
def test_estimate_floor_recovers_the_planted_plane(up_axis):
    from rohm_amd.floor import estimate_floor
    j, on, ref = planted()
    want = ref[up_axis]
    est = estimate_floor(_dev(j), hypotheses=512, seed=0, up_axis=up_axis)
    angle, off = FR.plane_errors(est)
    bar_angle, bar_off = bars(est)
    diff = max(np.abs(est.normal - want.normal).max(), abs(est.offset - want.offset))
    print(f'up {up_axis}: support {est.support} of {est.candidates}, extent {est.extent:.3f} m; angle {angle:.3e} rad (bar {bar_angle:.3e}), '
          f'height at the centroid {off:.3e} m (bar {bar_off:.3e}); against the restatement {diff:.3e} (bar 1e-10)')
    record('gpu', 'estimate_noisy_angle_over_bar', angle / bar_angle)
    record('gpu', 'estimate_noisy_offset_over_bar', off / bar_off)
    record('gpu', 'estimate_vs_restatement', diff)
    assert angle <= bar_angle and off <= bar_off
    assert diff <= 1e-10
    assert (est.candidates, est.support, est.under, est.hypothesis) == (want.candidates, want.support, want.under, want.hypothesis)
    assert np.abs(est.cam2world - want.cam2world).max() <= 1e-9 and est.up_axis == up_axis and est.floor_height == 0.0
    e = np.eye(3)[{'z': 2, 'y': 1}[up_axis]]
    assert np.abs(est.cam2world[:3, :3] @ est.normal - e).max() < 1e-12
    again = estimate_floor(_dev(j), hypotheses=512, seed=0, up_axis=up_axis)
    assert np.array_equal(again.normal, est.normal) and again.offset == est.offset and again.rms == est.rms
    other = estimate_floor(_dev(j), hypotheses=512, seed=5, up_axis=up_axis)
    assert np.abs(other.normal - est.normal).max() < 1e-9                            # another seed, the same inliers, the same plane


def test_estimate_floor_refuses():
    from rohm_amd.floor import estimate_floor
    j, on, _ = planted()
    with pytest.raises(ValueError, match='min_candidates=30'):
        estimate_floor(_dev(j[:24]), hypotheses=64)
    assert estimate_floor(_dev(j[:24]), hypotheses=64, strict=False).candidates == 24
    with pytest.raises(ValueError, match='min_support=0.9'):
        estimate_floor(_dev(j), hypotheses=64, min_support=0.9)
    with pytest.raises(ValueError, match='min_extent=5'):
        estimate_floor(_dev(j), hypotheses=64, min_extent=5)
    valid = np.ones(len(j), bool)
    valid[1::2] = False                                                              # every successor is two intervals away: beyond max_gap
    with pytest.raises(ValueError, match='a plane needs 3'):
        estimate_floor(_dev(j), valid=valid, max_gap=0.05, hypotheses=64)


def test_check_floor_on_a_known_rigid_motion():
    """The planted track seen from a calibrated camera: cam2world = (a turn about the up axis and a shift along the floor) .
    (the planted plane's own pose).  The floor is the world's z = 0."""
    from rohm_amd.floor import cam2world_from_plane, check_floor
    j, on, _ = planted()
    n, d = FR.planted_plane()
    c, s = np.cos(0.7), np.sin(0.7)
    move = np.array([[c, -s, 0.0, 1.5], [s, c, 0.0, -0.4], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
    cam2world = move @ cam2world_from_plane(n, d, 'z')
    est, angle_deg, height_diff = check_floor(_dev(j), cam2world, 'z', floor_height=0.0, hypotheses=512, seed=0)
    bar_angle, bar_off = bars(est)
    print(f'check_floor: angle {angle_deg:.5f} deg (bar {np.degrees(bar_angle):.5f}), height {height_diff:+.3e} m (bar {bar_off:.3e})')
    record('gpu', 'check_floor_angle_over_bar', np.radians(angle_deg) / bar_angle)
    record('gpu', 'check_floor_height_over_bar', abs(height_diff) / bar_off)
    assert np.radians(angle_deg) <= bar_angle and abs(height_diff) <= bar_off
    assert abs(np.radians(angle_deg) - FR.plane_errors(est)[0]) < 1e-9


# ---- 7. end to end with the synthetic body layer -------------------------------------------------------------------------------------------------
def _layer():
    from rohm_amd.body_model import SMPLXLayer
    return SMPLXLayer.from_tensors(synth.synthetic_smplx_tensors(0)).to(DEV)


@pytest.fixture(scope='module')
def body_dir(tmp_path_factory):
    """SMPLX_NEUTRAL.npz in the released layout from the synthetic model."""
    t = synth.synthetic_smplx_tensors(0)
    V = t['v_template'].shape[0]
    kt = np.stack([np.array(synth.SMPLX_PARENTS), np.arange(55)]).astype(np.int64)
    kt[0, 0] = 2 ** 32 - 1
    d = tmp_path_factory.mktemp('body')
    np.savez(str(d / 'SMPLX_NEUTRAL.npz'), v_template=t['v_template'].numpy(), shapedirs=t['shapedirs'].numpy(),
             posedirs=t['posedirs'].numpy().T.reshape(V, 3, 486), J_regressor=t['J_regressor'].numpy(), kintree_table=kt,
             weights=t['lbs_weights'].numpy(), f=np.zeros((4, 3), np.int64))
    return str(d)


@pytest.fixture(scope='module')
def logdir(tmp_path_factory):
    keep = VT.N_FRAMES
    VT.N_FRAMES = 8
    try:
        a = VT.synthetic_tree_arrays('prox', seed=0)
    finally:
        VT.N_FRAMES = keep
    return VT.write_tree(str(tmp_path_factory.mktemp('stats')), 'prox', a)['logdir']


STANCES, TRIES = 40, 16384


def sliding_body(seed=3):
    """A rigid body (zero pose, zero orientation, zero betas) that slides over a tilted plane through its own toe joints, with
    pauses: per stance three frames at rest, then two on the way (0.1 .. 0.3 m in a tenth of a second).  The plane's normal is
    perpendicular to the toe-to-toe vector and has most rest joints above it: the closed-form plane; it passes through toe 10
    of the untranslated body, so d = -n . rest[10].

    Noise-free has to be made: the joints are float32 out of `rohm_smplx_joints`.  (a) The rigid body the estimator sees is
    the device's: its rest joints (zero translation) differ from the layer's float64 regression by float32 rounding, 2e-8 m
    across the two toes, so the closed-form plane is taken from the device's rest joints, in float64.  (b) A float32
    position does not lie on a tilted plane -- half an ulp at 0.9 m is 3e-8 m, which moved the fitted plane by 2.9e-8 rad
    when the stops were taken as they came.  So every stop is chosen among `TRIES` float32 translations within a millimetre
    of where the walk wants it: the one for which both toes, as the device computes them, come closest to the plane.

    -> (track dict without cam2world, n, d, under_tol, worst): under_tol is the largest depth of a rest joint under the
    plane plus 1 cm (the synthetic body's feet are not its lowest joints), worst the largest distance of a resting toe to
    the plane."""
    from rohm_amd.body_model import native_for
    from rohm_amd.export import _joints
    nat = native_for(_layer(), torch.device(DEV))

    def fk(transl, sel=slice(None)):
        M = len(transl)
        with torch.cuda.device(nat.device):
            j = _joints(nat, torch.zeros(M, 22, 3, device=DEV), torch.zeros(M, 10, device=DEV), _dev(transl))
        return j[:, sel].cpu().numpy().astype(np.float64)
    rest = fk(np.zeros((1, 3), np.float32))[0]
    w = rest[11] - rest[10]
    w = w / np.linalg.norm(w)
    n = np.array([0.2, -0.3, 1.0])
    n = n - (n @ w) * w
    n = n / np.linalg.norm(n)
    height = (rest - rest[10]) @ n
    if (height < 0).sum() > (height > 0).sum():
        n, height = -n, -height
    d = float(-n @ rest[10])
    under_tol = float(max(0.0, -height.min()) + 0.01)
    u1, u2 = w, np.cross(n, w)
    g = np.random.Generator(np.random.PCG64(seed))
    heading = g.uniform(0, 2 * np.pi, size=STANCES)
    ab = np.cumsum(g.uniform(0.1, 0.3, size=(STANCES, 1)) * np.stack([np.cos(heading), np.sin(heading)], axis=1), axis=0)
    ab = ab - ab.mean(axis=0)
    ab = ab[:, None] + g.uniform(-1e-3, 1e-3, size=(STANCES, TRIES, 2))
    tries = (ab[..., :1] * u1 + ab[..., 1:] * u2).astype(np.float32).reshape(-1, 3)
    off = np.abs(fk(tries, slice(10, 12)) @ n + d).max(axis=1).reshape(STANCES, TRIES)
    pick = off.argmin(axis=1)
    stops = tries.reshape(STANCES, TRIES, 3)[np.arange(STANCES), pick]
    transl = []
    for m in range(STANCES):
        nxt = stops[min(m + 1, STANCES - 1)]
        transl += [stops[m]] * 3 + [stops[m] + (nxt - stops[m]) / 3.0, stops[m] + (nxt - stops[m]) * 2.0 / 3.0]
    transl = np.asarray(transl, dtype=np.float32)
    N = len(transl)
    track = dict(global_orient=np.zeros((N, 3), np.float32), transl=transl, body_pose=np.zeros((N, 63), np.float32), betas=np.zeros(10, np.float32),
                 fps=30.0, recording_name=np.array('slide'))
    return track, n, d, under_tol, float(off[np.arange(STANCES), pick].max())


@pytest.fixture(scope='module')
def slide(tmp_path_factory, body_dir):
    """`python -m rohm_amd.floor --track raw.npz --out calibrated.npz --json report.json` once, shared by the tests below."""
    from rohm_amd.floor import main
    track, n, d, under_tol, worst = sliding_body()
    root = tmp_path_factory.mktemp('slide')
    raw, out, js = str(root / 'raw.npz'), str(root / 'calibrated.npz'), str(root / 'report.json')
    np.savez(raw, **track)
    opts = ['--body_model_path', body_dir, '--under_tol', repr(under_tol), '--hypotheses', '256', '--seed', '0']
    assert main(['--track', raw, '--out', out, '--json', js] + opts) == 0
    with open(js) as f:
        rep = json.load(f)
    return dict(track=track, n=n, d=d, under_tol=under_tol, worst=worst, raw=raw, out=out, opts=opts, report=rep, root=root)


def test_cli_plane_is_the_closed_form_one(slide):
    from rohm_amd.floor import ESTIMATE_FIELDS
    est, n, d = slide['report']['estimate'], slide['n'], slide['d']
    got_n = np.asarray(est['normal'])
    angle = float(np.arctan2(np.linalg.norm(np.cross(n, got_n)), n @ got_n))
    print(f'end to end: {est["candidates"]} candidates, support {est["support"]}, under {est["under"]}, extent {est["extent"]:.3f} m, resting toes '
          f'within {slide["worst"]:.2e} m of the plane; angle to the closed-form plane {angle:.3e} rad, offset {abs(est["offset"] - d):.3e} m (bar 1e-9)')
    record('gpu', 'end_to_end_angle_rad', angle)
    record('gpu', 'end_to_end_offset_m', abs(est['offset'] - d))
    assert est['candidates'] == 2 * (2 * (STANCES - 1) + 4) and est['support'] == est['candidates'] and est['under'] == 0
    assert angle <= 1e-9 and abs(est['offset'] - d) <= 1e-9
    assert set(est) == set(ESTIMATE_FIELDS)
    assert slide['report']['options']['under_tol'] == slide['under_tol'] and slide['report']['options']['strict'] is True


def test_cli_output_is_a_track_every_consumer_accepts(slide, logdir):
    from rohm_amd.data_loaders.track import TRACK_KEYS, DataloaderTrack, read_track
    from rohm_amd.floor import calibrate_track
    track, est = slide['track'], slide['report']['estimate']
    with pytest.raises(ValueError, match='cam2world'):
        read_track(slide['raw'])                                                     # the track loader still refuses the raw file
    with np.load(slide['out'], allow_pickle=False) as f:
        cal = {k: f[k] for k in f.files}
    assert set(cal) <= set(TRACK_KEYS) and set(cal) == set(track) | {'cam2world', 'floor_height', 'up_axis'}
    rec = read_track(slide['out'])
    assert rec['up_axis'] == 'z' and rec['floor_height'] == 0.0 and np.array_equal(rec['cam2world'], np.asarray(est['cam2world']))
    ds = DataloaderTrack(slide['out'], body_model_path=_layer(), logdir=logdir, task='pose', clip_len=17, overlap_len=2,
                         use_scene_floor_height=True, device=DEV)
    assert len(ds) >= 10 and ds.scene_floor_height == 0.0
    # the same through the library, from a dict; up_axis and toe_height reach the file
    cal2, est2 = calibrate_track(track, _layer(), device=DEV, under_tol=slide['under_tol'], hypotheses=256, seed=0)
    assert set(cal2) == set(cal) and np.array_equal(cal2['cam2world'], cal['cam2world']) and est2.support == est['support']
    cal3, est3 = calibrate_track(track, _layer(), device=DEV, under_tol=slide['under_tol'], hypotheses=256, up_axis='y', toe_height=0.02)
    rec3 = read_track(cal3)
    assert rec3['up_axis'] == 'y' and rec3['floor_height'] == -0.02 and np.abs(cal3['cam2world'][:3, :3] @ est3.normal - [0, 1, 0]).max() < 1e-12


def test_cli_check_and_refusals(slide, capsys):
    from rohm_amd.floor import main
    root, opts = slide['root'], slide['opts']
    js = str(root / 'check.json')
    assert main(['--track', slide['out'], '--check', '--json', js] + opts) == 0
    text = capsys.readouterr().out
    assert 'the floor of this track' in text and 'given cam2world' in text and 'wrote' not in text
    with open(js) as f:
        chk = json.load(f)['check']
    print(f'--check on the output: {chk["angle_deg"]:.3e} deg, {chk["height_diff"]:+.3e} m (bar 1e-6)')
    assert chk['angle_deg'] < 1e-6 and abs(chk['height_diff']) < 1e-6
    with pytest.raises(SystemExit, match='has none'):
        main(['--track', slide['raw'], '--check'] + opts)
    # a body that stands still cannot be calibrated
    track = slide['track']
    still = dict(track, transl=np.repeat(track['transl'][:1], len(track['transl']), axis=0))
    np.savez(str(root / 'still.npz'), **still)
    with pytest.raises(SystemExit, match='one line'):
        main(['--track', str(root / 'still.npz'), '--out', str(root / 'no.npz')] + opts)
    assert not os.path.exists(str(root / 'no.npz'))


