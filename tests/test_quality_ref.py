"""CPU: the numpy restatement of csrc/quality.hip (tests/quality_ref.py) on cases that can be computed by hand, `TrackQuality`'s
host side (`worst`, `summary`) on hand-made rows, and the refusals of `python -m rohm_amd.quality` that need no device."""
import pickle

import numpy as np
import pytest

import quality_ref as QR
from rohm_amd import quality as Q


def _standing_body(n, seed=0):
    """n frames of one random body about 1 m in size, its four foot joints exactly at height 0 (z up)."""
    g = np.random.Generator(np.random.PCG64(seed))
    body = g.uniform(-0.5, 0.5, size=(22, 3)).astype(np.float32)
    body[:, 2] += 1.0
    body[list(QR.FOOT), 2] = 0.0
    return np.repeat(body[None], n, axis=0)


def test_a_sliding_body_skates_in_every_pair():
    n = 12
    j = _standing_body(n)
    j[:, :, 0] += (np.arange(n, dtype=np.float32) * np.float32(0.2 / 30.0))[:, None]          # 0.2 m/s along x
    rows, tot = QR.track_quality(j, 30.0, 2, True, 0.0)
    assert rows[:-1, 3].tolist() == [1.0] * (n - 1) and np.isnan(rows[-1, 3])
    assert tot[0, 4] == n - 1 and tot[0, 5] == n - 1 and tot[0, 0] == n and tot[1, 0] == 0 and np.isnan(tot[1, 3])
    assert (rows[:, 5] == 0.0).all() and tot[0, 8] == 0 and tot[0, 10] == 2 * n            # on the floor, not under it
    # the same body 0.05 m/s: too slow to skate; lifted 0.2 m: too high; without a floor: not scored
    slow = _standing_body(n)
    slow[:, :, 0] += (np.arange(n, dtype=np.float32) * np.float32(0.05 / 30.0))[:, None]
    assert not QR.track_quality(slow, 30.0, 2, True, 0.0)[0][:-1, 3].any()
    assert not QR.track_quality(j, 30.0, 2, True, -0.2)[0][:-1, 3].any()
    rows, tot = QR.track_quality(j, 30.0, 2, False, 0.0)
    assert np.isnan(rows[:, 3]).all() and np.isnan(rows[:, 5]).all() and tot[0, 5] == 0 and tot[0, 10] == 0
    # y up: the same track with y and z exchanged
    rows_y, tot_y = QR.track_quality(j[:, :, [0, 2, 1]], 30.0, 1, True, 0.0)
    assert rows_y[:-1, 3].all() and tot_y[0, 4] == n - 1
    # one toe 8 cm under the floor in frame 3: pene, the count below -0.05 and the sum
    j[3, 10, 2] = -0.08
    rows, tot = QR.track_quality(j, 30.0, 2, True, 0.0)
    assert rows[3, 5] == np.float64(np.float32(-0.08)) and tot[0, 8] == 1 and tot[0, 9] == np.float64(np.float32(-0.08))


def test_constant_velocity_has_zero_acceleration():
    n = 9
    j = _standing_body(n, 1)
    step = np.float32(2.0 ** -6)                                                              # on a grid of 1 / 64 m every sum is exact
    j = (np.round(j * 64) / 64).astype(np.float32)
    j[:, :, 1] += (np.arange(n, dtype=np.float32) * step)[:, None]
    rows, tot = QR.track_quality(j, 30.0, 2, True, 0.0)
    assert (rows[:-2, 4] == 0.0).all() and np.isnan(rows[-2:, 4]).all() and tot[0, 6] == 0.0 and tot[0, 7] == n - 2
    # one joint displaced by 1 / 64 m in one frame: |a| = 900 / 64 in the frames before and after, twice that at the frame itself
    j[4, 3, 0] += np.float32(0.015625)
    rows, _ = QR.track_quality(j, 30.0, 2, True, 0.0)
    want = 0.015625 * 900.0 / 22.0
    assert np.allclose(rows[[2, 4], 4], want, rtol=1e-12) and np.isclose(rows[3, 4], 2 * want, rtol=1e-12) and rows[5, 4] == 0.0


def test_own_projection_has_residual_zero():
    n = 5
    j = _standing_body(n, 2)
    c, s = np.cos(0.3), np.sin(0.3)
    scene2cam = np.array([[c, 0, s, 0.1], [0, 1, 0, -0.2], [-s, 0, c, 3.0], [0, 0, 0, 1.0]])
    cam = (1000.0, 990.0, 960.0, 540.0)
    uv, Z, _ = QR.project(j, scene2cam, *cam)
    assert (Z > 1.0).all()
    kp = np.concatenate([uv, np.full((n, 22, 1), 0.9)], axis=-1)                              # float64: exactly the projection
    rows, tot = QR.track_quality(j, 30.0, 2, True, 0.0, scene2cam, *cam, keypoints=kp.astype(np.float64))
    # the restatement rounds keypoints to float32, as the kernel reads them: the residual is that rounding, below 1e-4 px
    assert (rows[:, 0] < 1e-4).all() and (rows[:, 1] < 2e-4).all() and (rows[:, 2] == 22).all() and tot[0, 2] == n
    # a keypoint 3 px to the right and 4 px down at confidence 0.5 among 21 exact ones at 0.9: 5 px * 0.5 / (0.5 + 21 * 0.9)
    kp32 = kp.astype(np.float32)
    exact = QR.track_quality(j, 30.0, 2, True, 0.0, scene2cam, *cam, keypoints=kp32)[0]
    kp32[2, 7, :2] += np.float32([3.0, 4.0])
    kp32[2, 7, 2] = 0.5
    rows, _ = QR.track_quality(j, 30.0, 2, True, 0.0, scene2cam, *cam, keypoints=kp32)
    assert abs(rows[2, 1] - 5.0) < 1e-3 and abs(rows[2, 0] - 5.0 * 0.5 / (0.5 + 21 * 0.9)) < 1e-3 and np.array_equal(rows[3], exact[3], equal_nan=True)
    # confidences at or below conf_min, and joints behind the camera, do not count; nothing left: NaN
    kp32[1, :, 2] = 0.2
    kp32[3, :5, 2] = 0.0
    rows, tot = QR.track_quality(j, 30.0, 2, True, 0.0, scene2cam, *cam, keypoints=kp32, conf_min=0.2)
    assert np.isnan(rows[1, :2]).all() and rows[1, 2] == 0 and rows[3, 2] == 17 and tot[0, 2] == n - 1
    behind = scene2cam.copy()
    behind[2, 3] = -3.0
    rows, tot = QR.track_quality(j, 30.0, 2, True, 0.0, behind, *cam, keypoints=kp32)
    assert np.isnan(rows[:, 0]).all() and not rows[:, 2].any() and tot[0, 2] == 0 and np.isnan(tot[0, 3])


def test_deviation_groups_and_nan_rules():
    n = 6
    j = _standing_body(n, 3)
    ref = j.copy()
    ref[:, :, 0] += np.float32(0.25)                                                           # 25 cm away, every joint
    mask = np.ones((n, 22), np.float32)
    mask[1] = 0.0
    mask[2, :11] = 0.0
    gap = np.array([0, 0, 1, 1, 0, 0], np.uint8)
    rows, tot = QR.track_quality(j, 30.0, 2, True, 0.0, joints_ref=ref, mask_ref=mask, gap=gap)
    assert np.allclose(rows[[0, 2, 3, 4, 5], 6], 0.25, rtol=1e-6) and np.isnan(rows[1, 6])
    assert np.allclose(rows[[1, 2], 7], 0.25, rtol=1e-6) and np.isnan(rows[[0, 3, 4, 5], 7]).all()
    assert rows[:, 8].tolist() == [22, 0, 11, 22, 22, 22] and rows[:, 9].tolist() == gap.tolist()
    assert tot[:, 0].tolist() == [4, 2] and tot[:, 12].tolist() == [3, 2] and tot[:, 14].tolist() == [1, 1]
    assert tot[:, 7].tolist() == [2, 2] and tot[:, 5].tolist() == [3, 2]                       # triples (0, 1 | 2, 3), pairs (0, 1, 4 | 2, 3)
    assert np.array_equal(tot, QR.totals_from(rows, j[:, list(QR.TOES), 2].astype(np.float64)), equal_nan=True)
    # a NaN joint reaches exactly what reads it
    base = QR.track_quality(j, 30.0, 2, True, 0.0, joints_ref=ref, mask_ref=mask, gap=gap)[0]
    bad = j.copy()
    bad[3, 10] = np.nan                                                                         # a toe of frame 3
    rows = QR.track_quality(bad, 30.0, 2, True, 0.0, joints_ref=ref, mask_ref=mask, gap=gap)[0]
    changed = ~((rows == base) | (np.isnan(rows) & np.isnan(base)))
    want = np.zeros_like(changed)
    want[[1, 2, 3], 4] = True
    want[[2, 3], 3] = True
    want[3, [5, 6]] = True
    assert np.array_equal(changed, want) and np.isnan(rows[changed]).all()


def test_floor_clearance_restatement():
    v = np.zeros((2, 5, 3), np.float32)
    v[0, :, 2] = [0.3, -0.1, 0.2, -0.1, -0.02]
    v[1, :, 2] = [0.5, 0.4, 0.4, 0.6, 0.7]
    out = QR.floor_clearance(v, 2, -0.02, 0.05)
    assert out[0].tolist() == [np.float64(np.float32(-0.1)) - np.float64(np.float32(-0.02)), 1.0, 2.0]
    assert out[1, 1] == 1.0 and out[1, 2] == 0.0
    v[1, 2, 2] = np.nan
    assert np.isnan(QR.floor_clearance(v, 2, 0.0)[1, [0, 2]]).all() and QR.floor_clearance(v, 2, 0.0)[1, 1] == -1.0


def _hand_rows():
    rows = np.zeros((20, 10))
    rows[:, 0] = [1, 1, 8, 9, 10, 6, 1, 1, 1, 4, 1, 1, np.nan, 7, 7, np.nan, 1, 1, 1, 1]
    rows[:, 5] = 0.0
    rows[5:8, 5] = [-0.02, -0.08, -0.05]
    rows[:, 3] = 0.0
    rows[10:13, 3] = 1.0
    return rows


def test_worst_ranges_on_hand_made_rows():
    q = Q.TrackQuality(_hand_rows(), np.zeros((2, 15)))
    assert len(q) == 20
    # the peak 10 takes its neighbours down to half of it (5): frames 2 .. 5; then 7, 7 between two NaN frames; then 4 alone
    assert q.worst('reproj_px', 3) == [(2, 6, 10.0), (13, 15, 7.0), (9, 10, 4.0)]
    assert q.worst('reproj_px', 1) == [(2, 6, 10.0)] and q.worst(0, 3, min_len=2) == [(2, 6, 10.0), (13, 15, 7.0), (0, 2, 1.0)]
    assert q.worst('pene', 5) == [(6, 8, -0.08), (5, 6, -0.02)]                             # the most negative is the worst
    assert q.worst('skate', 5) == [(10, 13, 1.0)] and q.worst('accel', 5) == []
    with pytest.raises(ValueError):
        q.worst('no_such_column')


def test_summary_names_and_units():
    tot = np.zeros((2, 15))
    tot[0] = [10, 30.0, 6, 9.0, 2, 8, 16.0, 8, 1, -0.2, 20, 0.5, 10, 0.0, 0]
    tot[1] = [2, 0.0, 0, np.nan, 0, 2, 4.0, 2, 0, 0.0, 4, 0.0, 0, 0.6, 2]
    q = Q.TrackQuality(np.zeros((12, 10)), tot)
    s = q.summary()
    assert set(s) == {'observed', 'infilled', 'all'}
    o, i, a = s['observed'], s['infilled'], s['all']
    assert o['reproj_px'] == 5.0 and o['reproj_max_px'] == 9.0 and o['skating'] == 0.25 and o['acc'] == 2.0
    assert o['ground_pene_freq'] == 5.0 and abs(o['ground_pene_dist'] - 10.0) < 1e-12 and o['dev_vis_mm'] == 50.0 and np.isnan(o['dev_occ_mm'])
    assert np.isnan(i['reproj_px']) and np.isnan(i['reproj_max_px']) and i['frames_reproj'] == 0 and i['dev_occ_mm'] == 300.0
    assert a['frames'] == 12 and a['reproj_max_px'] == 9.0 and a['skating'] == 0.2 and a['acc'] == 2.0 and a['dev_occ_mm'] == 300.0
    from rohm_amd.evaluation import SceneMetrics
    shared = set(SceneMetrics('prox', 10, np.zeros((1, 11))).summary())
    assert shared == {'skating', 'acc', 'ground_pene_freq', 'ground_pene_dist'} and shared <= set(o)
    assert len(q.lines()) == 9 and q.lines()[0].startswith('reproj (px):') and q.lines()[0].endswith('5.00 / nan')


def test_main_refusals(tmp_path):
    with pytest.raises(SystemExit, match='one of --saved_data_dir and --saved_data_path'):
        Q.main(['--track', 'x.npz'])
    with pytest.raises(SystemExit, match='one of --saved_data_dir and --saved_data_path'):
        Q.main(['--track', 'x.npz', '--saved_data_dir', 'a', '--saved_data_path', 'b'])
    with pytest.raises(SystemExit, match='--track'):
        Q.main(['--saved_data_path', 'b.pkl'])
    # a PROX / EgoBody result pickle has no clip_starts: refused with a message that says so, before any device is touched
    p = tmp_path / 'prox.pkl'
    with open(p, 'wb') as f:
        pickle.dump({'motion_repr_rec_list': np.zeros((1, 15, 294), np.float32), 'recording_name': 'N0Sofa'}, f)
    with pytest.raises(SystemExit, match='not a track pickle'):
        Q.main(['--saved_data_path', str(p), '--track', 'x.npz'])
    with pytest.raises(ValueError, match='clip_starts'):
        Q.load_track_pickle({'motion_repr_rec_list': 0})
    with pytest.raises(ValueError, match='mask_joint_vis_list'):
        Q.load_track_pickle({'clip_starts': [0], 'times_dst': 0, 'gap': 0, 'motion_repr_rec_list': 0, 'motion_repr_noisy_list': 0,
                             'trans_scene2cano_list': 0})
    with pytest.raises(TypeError, match='HIP device'):
        Q.track_quality(np.zeros((3, 22, 3), np.float32))
    import torch
    from rohm_amd._lib import RohmHipError
    with pytest.raises(RohmHipError, match='no CPU fallback'):
        Q.track_quality(torch.zeros(3, 22, 3))
