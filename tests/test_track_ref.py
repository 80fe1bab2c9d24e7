"""CPU: the numpy restatement of the track resampling rule (tests/track_ref.py) -- its slerp against scipy, copy-through,
gaps and holds -- and the host side of rohm_amd/data_loaders/track.py: `plan_times`, `plan_windows`, `frames_plan`,
`read_track` and its refusals."""
import numpy as np
import pytest

import track_ref as TR
from rohm_amd.data_loaders import track as T


def _pairs(n, seed=0):
    """n pairs of rotation vectors: angles at most 3.0 rad, relative rotation at most 2.0 rad."""
    g = np.random.Generator(np.random.PCG64(seed))
    r0 = TR.random_rotvecs(g, (3 * n,), 3.0)
    r1 = TR.compose(r0, TR.random_rotvecs(g, (3 * n,), 2.0))
    keep = np.flatnonzero(np.linalg.norm(r1, axis=-1) <= 3.0)[:n]
    assert len(keep) == n
    return r0[keep], r1[keep], g.uniform(0.0, 1.0, size=n)


def test_slerp_against_scipy():
    from scipy.spatial.transform import Rotation, Slerp
    n = 20000
    r0, r1, alpha = _pairs(n)
    assert TR.geodesic(r0, r1).max() <= 2.0 + 1e-9
    seq = np.stack([r0, r1], axis=1).reshape(2 * n, 3)                   # a0 b0 a1 b1 ...: pair k lives on [2k, 2k + 1]
    t = 2.0 * np.arange(n) + alpha
    alpha = t - 2.0 * np.arange(n)                                       # the fraction scipy sees: t has lost low bits of alpha
    ref = Slerp(np.arange(2 * n, dtype=np.float64), Rotation.from_rotvec(seq))(t)
    got = Rotation.from_rotvec(TR.slerp_rotvec(r0, r1, alpha))
    err = (ref.inv() * got).magnitude()
    print(f'slerp restatement vs scipy: max geodesic {err.max():.3e} rad (bar 1e-12)')
    assert err.max() <= 1e-12
    # the restatement's own geodesic agrees with scipy's
    assert np.abs(TR.geodesic(ref.as_rotvec(), got.as_rotvec()) - err).max() <= 1e-12
    # the end points, and the shortest arc for an antipodal quaternion pair
    assert TR.geodesic(TR.slerp_rotvec(r0, r1, np.zeros(n)), r0).max() <= 1e-12
    assert TR.geodesic(TR.slerp_rotvec(r0, r1, np.ones(n)), r1).max() <= 1e-12
    assert np.linalg.norm(TR.slerp_rotvec(r0, r1, alpha), axis=-1).max() <= np.pi + 1e-12
    same = TR.slerp_rotvec(r0[:5], r0[:5], alpha[:5])                    # omega = 0: the lerp weights
    assert TR.geodesic(same, r0[:5]).max() <= 1e-12


def _track(n=12, fps=25.0, seed=1, J=22, M=25):
    g = np.random.Generator(np.random.PCG64(seed))
    params = TR.smooth_params(g, n)
    kp = np.concatenate([g.uniform(size=(n, J, 2)) * np.array([1920.0, 1080.0]), g.uniform(0.1, 1.0, size=(n, J, 1))], -1).astype(np.float32)
    mask = (g.uniform(size=(n, M)) > 0.3).astype(np.float32)
    return np.arange(n) / fps, params, kp, mask


def test_copy_through_is_the_source_bits():
    ts, params, kp, mask = _track()
    valid = np.ones(12, bool)
    valid[5] = False
    td = np.array([ts[0], ts[3], ts[4], ts[6], ts[11]])
    r = TR.resample(ts, valid, params, kp, mask, td, 10.0)
    src = [0, 3, 4, 6, 11]
    assert r['src_index'].tolist() == src and not r['gap'].any()
    assert r['params'].tobytes() == params[src].tobytes()
    assert r['keypoints'].tobytes() == kp[src].tobytes() and r['mask_joint'].tobytes() == mask[src].tobytes()
    # 60 fps -> 30 fps: every output time is a source time
    ts60 = np.arange(12) / 60.0
    td = TR.plan_times(ts60, np.ones(12, bool))
    assert len(td) == 6 and np.array_equal(td, ts60[::2])
    r = TR.resample(ts60, np.ones(12, bool), params, kp, mask, td, 0.025)
    assert r['params'].tobytes() == params[::2].tobytes() and r['src_index'].tolist() == [0, 2, 4, 6, 8, 10]


def test_gaps_and_holds():
    ts, params, kp, mask = _track()
    kp[3, 4, 2] = 0.0                                                     # one missed detection in a valid frame
    valid = np.ones(12, bool)
    valid[[0, 5, 6, 11]] = False                                          # leading, inner (two frames) and trailing
    td = np.array([0.0, 0.05, 0.13, 0.17, 0.21, 0.25, 0.30, 0.41, 0.44, 0.5])
    r = TR.resample(ts, valid, params, kp, mask, td, 0.06)
    assert r['src_index'].tolist() == [1, 1, 3, 4, 4, 4, 7, 10, 10, 10]
    assert r['gap'].tolist() == [1, 0, 0, 1, 1, 1, 0, 1, 1, 1]
    gap = r['gap'].astype(bool)
    # holds: the nearest valid row's parameters; no evidence
    assert r['params'][0].tobytes() == params[1].tobytes() and r['params'][-1].tobytes() == params[10].tobytes()
    assert r['params'][7].tobytes() == params[10].tobytes()               # 0.41 is past 0.40, the last valid time
    assert not r['keypoints'][gap].any() and not r['mask_joint'][gap].any()
    # inside the inner gap the parameters are interpolated between frames 4 and 7
    a = (0.21 - ts[4]) / (ts[7] - ts[4])
    assert np.abs(r['params'][4, 3:16] - (params[4, 3:16] + a * (params[7, 3:16] - params[4, 3:16]))).max() <= 1e-15
    assert TR.geodesic(r['params'][4, 0:3], TR.slerp_rotvec(params[4, 0:3], params[7, 0:3], a)) <= 1e-12
    assert 0 < TR.geodesic(r['params'][4, 0:3], params[4, 0:3]) < TR.geodesic(params[7, 0:3], params[4, 0:3])
    # outside a gap: min of confidences and masks, a missed detection takes the other bracket's position
    k = 2                                                                 # t = 0.13 between frames 3 and 4
    assert np.array_equal(r['keypoints'][k, :, 2], np.where(np.arange(22) == 4, 0, np.minimum(kp[3, :, 2], kp[4, :, 2])))
    assert np.array_equal(r['keypoints'][k, 4, :2], kp[4, 4, :2])
    assert np.array_equal(r['mask_joint'][k], np.minimum(mask[3], mask[4]))
    al = (0.13 - ts[3]) / (ts[4] - ts[3])
    want = (kp[3, 0, :2].astype(np.float64) + al * (kp[4, 0, :2].astype(np.float64) - kp[3, 0, :2])).astype(np.float32)
    assert np.array_equal(r['keypoints'][k, 0, :2], want)
    # without keypoints and masks
    r2 = TR.resample(ts, valid, params, None, None, td, 0.06)
    assert r2['keypoints'] is None and r2['mask_joint'] is None and r2['params'].tobytes() == r['params'].tobytes()


def test_plans():
    assert T.plan_windows(20, 8, 2).tolist() == TR.plan_windows(20, 8, 2) == [0, 6, 12]
    assert T.plan_windows(23, 8, 2).tolist() == TR.plan_windows(23, 8, 2) == [0, 6, 12, 15]
    assert T.plan_windows(23, 8, 2, tail='drop').tolist() == TR.plan_windows(23, 8, 2, 'drop') == [0, 6, 12]
    assert T.plan_windows(8, 8, 2).tolist() == [0] and T.plan_windows(9, 8, 2).tolist() == [0, 1]
    with pytest.raises(ValueError, match=r'0\.233 s'):
        T.plan_windows(7, 8, 2)
    with pytest.raises(ValueError):
        T.plan_windows(20, 8, 2, tail='pad')
    for fps, n in ((25.0, 37), (30.0, 20), (60.0, 41)):
        ts = np.arange(n) / fps
        valid = np.ones(n, bool)
        if fps == 25.0:
            valid[[0, n - 1]] = False
        td = T.plan_times(ts, valid)
        assert np.array_equal(td, TR.plan_times(ts, valid))
        tv = ts[valid]
        assert td[0] == tv[0] and td[-1] <= tv[-1] + 1e-9 and td[-1] + 1 / 30.0 > tv[-1] + 1e-9
        assert np.array_equal(td, np.array([tv[0] + k / 30.0 for k in range(len(td))]))
    assert len(T.plan_times(np.arange(37) / 25.0, np.ones(37, bool))) == 44            # 1.44 s: 43.2 intervals
    assert np.array_equal(T.plan_times(np.arange(20) / 30.0, np.ones(20, bool)), np.arange(20) / 30.0)
    assert np.array_equal(T.plan_times(np.arange(41) / 60.0, np.ones(41, bool)), (np.arange(41) / 60.0)[::2])
    # the export plan of explicit starts: every frame once, earliest or latest clip
    fc, ft, n = T.frames_plan([0, 6, 12, 15], 8)
    assert n == 23 and (np.asarray([0, 6, 12, 15])[fc] + ft).tolist() == list(range(23))
    assert fc.tolist() == [0] * 8 + [1] * 6 + [2] * 6 + [3] * 3
    fc, ft, n = T.frames_plan([0, 6, 12, 15], 8, keep='last')
    assert fc.tolist() == [0] * 6 + [1] * 6 + [2] * 3 + [3] * 8 and (np.asarray([0, 6, 12, 15])[fc] + ft).tolist() == list(range(23))
    from rohm_amd.export import plan_frames
    for keep in ('first', 'last'):
        a, b = T.frames_plan([0, 6, 12], 6, keep), plan_frames(3, 6, 8, 2, keep)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    with pytest.raises(ValueError, match='uncovered'):
        T.frames_plan([0, 9], 8)


def _track_dict(n=10):
    ts, params, kp, mask = _track(n)
    return {'global_orient': params[:, 0:3].astype(np.float32), 'transl': params[:, 3:6].astype(np.float32),
            'betas': params[0, 6:16].astype(np.float32), 'body_pose': params[:, 16:79].astype(np.float32),
            'cam2world': np.eye(4), 'fps': 25.0, 'keypoints_2d': kp, 'mask_joint': mask}


def test_read_track(tmp_path):
    d = _track_dict()
    rec = T.read_track(d)
    assert rec['params79'].shape == (10, 79) and rec['params79'].dtype == np.float64 and rec['valid'].all()
    assert np.array_equal(rec['times'], np.arange(10) / 25.0) and rec['up_axis'] == 'z' and rec['floor_height'] is None
    assert np.array_equal(rec['params']['betas'], np.repeat(d['betas'][None], 10, 0)) and rec['params']['betas'].dtype == np.float32
    assert np.array_equal(rec['params79'][:, 0:3], d['global_orient'].astype(np.float64))
    assert rec['frame_names'][3] == 'frame_000003' and not rec['undistort'] and not rec['has_keypoints']      # no intrinsics given
    # BODY_25 keypoints go through OPENPOSE_TO_SMPL; an .npz file reads the same
    from rohm_amd.data_loaders.dataloader_video import OPENPOSE_TO_SMPL
    g = np.random.Generator(np.random.PCG64(3))
    kp25 = g.uniform(size=(10, 25, 3)).astype(np.float32)
    d25 = dict(d, keypoints_2d=kp25, camera_mtx=np.array([[1000.0, 0, 960], [0, 1000, 540], [0, 0, 1]]), dist_coeffs=np.zeros(5),
               up_axis='y', floor_height=-0.3, recording_name='walk', frame_names=np.array(['f%02d' % i for i in range(10)]))
    path = str(tmp_path / 'walk.npz')
    np.savez(path, **d25)
    rec = T.read_track(path)
    assert np.array_equal(rec['keypoints'], kp25[:, OPENPOSE_TO_SMPL[:22]]) and rec['up_axis'] == 'y' and rec['floor_height'] == -0.3
    assert rec['undistort'] and rec['has_keypoints'] and rec['color_cam']['f'] == [1000.0, 1000.0] and rec['color_cam']['c'] == [960.0, 540.0]
    assert rec['recording_name'] == 'walk' and rec['frame_names'][9] == 'f09'
    # a NaN row becomes invalid, not an error; so does a row the caller marks
    bad = dict(d)
    bad['transl'] = d['transl'].copy()
    bad['transl'][4, 1] = np.nan
    bad['valid'] = np.arange(10) != 7
    rec = T.read_track(bad)
    assert rec['valid'].tolist() == [i not in (4, 7) for i in range(10)] and np.isfinite(rec['params79']).all()
    # explicit times
    tt = dict(d)
    del tt['fps']
    tt['times'] = np.cumsum(np.full(10, 0.04)) + 3.0
    assert np.array_equal(T.read_track(tt)['times'], tt['times'])


def test_read_track_refusals():
    d = _track_dict()
    no_cam = dict(d)
    del no_cam['cam2world']
    with pytest.raises(ValueError, match='cam2world'):
        T.read_track(no_cam)
    with pytest.raises(ValueError, match='exactly one of fps and times'):
        T.read_track(dict(d, times=np.arange(10) / 25.0))
    neither = dict(d)
    del neither['fps']
    with pytest.raises(ValueError, match='exactly one of fps and times'):
        T.read_track(neither)
    t = np.arange(10) / 25.0
    t[5] = t[4]
    with pytest.raises(ValueError, match='strictly increasing'):
        T.read_track(dict(neither, times=t))
    for key, val in (('transl', d['transl'][:9]), ('body_pose', d['body_pose'][:, :60]), ('betas', np.zeros((10, 9))),
                     ('keypoints_2d', d['keypoints_2d'][:, :21]), ('mask_joint', d['mask_joint'][:, :21]), ('valid', np.ones(9, bool)),
                     ('cam2world', np.eye(3)), ('times', None)):
        bad = dict(neither, times=np.arange(9) / 25.0) if key == 'times' else dict(d, **{key: val})
        with pytest.raises(ValueError):
            T.read_track(bad)
    with pytest.raises(ValueError, match='no valid frame'):
        T.read_track(dict(d, valid=np.zeros(10, bool)))
    nan = dict(d, transl=np.full((10, 3), np.nan, np.float32))
    with pytest.raises(ValueError, match='no valid frame'):
        T.read_track(nan)
    with pytest.raises(ValueError, match='unknown keys'):
        T.read_track(dict(d, gender='male'))
    with pytest.raises(ValueError, match='up_axis'):
        T.read_track(dict(d, up_axis='x'))
    with pytest.raises(ValueError, match='go together'):
        T.read_track(dict(d, camera_mtx=np.eye(3)))
