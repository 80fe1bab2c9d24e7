"""CPU: the rule of the multi-view triangulation.  tests/multiview_ref.py (the float64 restatement tests/test_gpu_multiview.py
holds csrc/multiview.hip to) against closed forms, central differences and the recovery of planted points, and the host logic of
`rohm_amd.multiview` (`read_views`, `pack_cameras`, `triangulate_views`) with the two kernels replaced by the restatement.

Bars.  Closed-form intersection 1e-12 m and noise-free recovery 1e-9 m (float64 keypoints, `as_given`; no distortion): the
cofactor solves lose about cond x 1e-16, cond <= 1 / sin^2 of the rays' angle.  Round trip distort(undistort(p)): the
fixed-point map contracts by q <= 3 |k1| r^2 + 6 |p| r + ... per iteration; at the rig's strongest lens (|k1| <= 0.156,
|p| <= 0.0013) and r <= 0.3 that is q <= 0.05 on a first error of at most |k1| r^3 f = 4.2 px, so five iterations leave at
most 4.2 x 0.05^5 = 1.3e-6 px: the bar is ROUND_TRIP_PX = 1e-5 px (measured: 3.8e-8 px).  Jacobian against central
differences (step 1e-6 m): 1e-4 px/m on entries of order f / z = 250 px/m; the differences are good to f 1e-16 / 1e-6 = 1e-7
and their truncation to f h^2 / z^3 = 1e-11.  Noise: |X_hat - X| <= 5 x 2 px x sigma_m, the issue's bar (the largest measured
ratio to 2 px x sigma_m: 3.0).  Planted outliers 60 .. 300 px off are never inliers at tau_px = 10."""
import numpy as np
import pytest
import torch

import multiview_ref as MR
from rohm_amd import fit, multiview

ROUND_TRIP_PX = 1e-5


def rig(V, seed, distortion=False, **kw):
    return multiview.pack_cameras(*MR.make_rig(V, seed, distortion, **kw))


def exact_keypoints(cams, X, conf=1.0):
    """Float64 detections of X [N,J,3] in every view, confidence `conf`."""
    px, _ = MR.project(cams, X.reshape(-1, 3))
    kp = np.concatenate([px, np.full(px.shape[:2] + (1,), conf)], -1)
    return kp.reshape((cams.shape[0],) + X.shape[:2] + (3,))


def test_two_orthogonal_cameras_meet_at_the_intersection():
    # camera 0 at the origin looking along world z, camera 1 at (5, 0, 5) looking along world -x: their axes meet at (0, 0, 5)
    K = np.array([[[900.0, 0, 640], [0, 900.0, 360], [0, 0, 1]]] * 2)
    W = np.stack([np.eye(4), np.eye(4)])
    R1 = np.array([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]])
    W[1, :3, :3], W[1, :3, 3] = R1, -R1 @ np.array([5.0, 0, 5])
    cams = multiview.pack_cameras(K, W)
    # the rays through pixels (640 + 90, 360 - 45) and (640 + 180, 360 - 45): X = (0.5, -0.25, 5) + ..., solved by hand: camera 0
    # sees X at (x / z, y / z) = (0.1, -0.05); camera 1 sees it at ((z - 5) / (5 - x), y / (5 - x))
    X = np.array([0.5, -0.25, 5.0])
    kp = np.array([[[[640 + 900 * 0.1, 360 - 900 * 0.05, 1.0]]], [[[640 + 900 * (X[2] - 5) / (5 - X[0]), 360 + 900 * X[1] / (5 - X[0]), 1.0]]]])
    for refine in (0, 3):
        r = MR.triangulate(kp, cams, refine=refine, as_given=True)
        assert np.abs(r['joints'][0, 0] - X).max() <= 1e-12
        assert r['report'][0, 0, 0] == 2 and r['report'][0, 0, 3] == 2 and r['inliers'][0, 0] == 3
        assert r['report'][0, 0, 1] <= 1e-9
    rg = np.concatenate([R1.reshape(9), W[1, :3, 3]])
    r = MR.triangulate(kp, cams, rigid=rg, as_given=True)
    assert np.abs(r['joints'][0, 0] - (R1 @ X + W[1, :3, 3])).max() <= 1e-12


def test_distort_of_undistort_round_trip():
    cams = rig(5, 3, distortion=True)
    g = np.random.Generator(np.random.PCG64(4))
    ang, rad = g.uniform(0, 2 * np.pi, (5, 400)), 0.3 * np.sqrt(g.uniform(0, 1, (5, 400)))
    px, py = MR.distort(cams, rad * np.cos(ang), rad * np.sin(ang))
    a, b = MR.undistort(cams, px, py)
    qx, qy = MR.distort(cams, a, b)
    worst = float(np.hypot(qx - px, qy - py).max())
    print(f'round trip over r <= 0.3: {worst:.3e} px')
    assert worst <= ROUND_TRIP_PX
    assert np.hypot(a - rad * np.cos(ang), b - rad * np.sin(ang)).max() * 1030.0 <= ROUND_TRIP_PX
    plain = cams.copy()
    plain[:, 16:21] = 0.0
    a0, b0 = MR.undistort(plain, px, py)
    assert np.array_equal(a0, (px - plain[:, 14:15]) / plain[:, 12:13]) and np.array_equal(b0, (py - plain[:, 15:16]) / plain[:, 13:14])


def test_jacobian_against_central_differences():
    cams = rig(4, 5, distortion=True)
    g = np.random.Generator(np.random.PCG64(6))
    X = np.array([0.0, 0.0, 1.0]) + g.uniform(-0.6, 0.6, (50, 3))
    a, b = g.uniform(-0.2, 0.2, 50), g.uniform(-0.2, 0.2, 50)
    h = 1e-6
    for v in range(4):
        _, _, J = MR.residual(cams[v], X, a, b, with_j=True)
        for k in range(3):
            dX = np.zeros(3)
            dX[k] = h
            rp, _ = MR.residual(cams[v], X + dX, a, b)
            rm, _ = MR.residual(cams[v], X - dX, a, b)
            assert np.abs((rp - rm) / (2 * h) - J[..., k]).max() <= 1e-4


@pytest.mark.parametrize('V', [2, 3, 5, 16])
def test_noise_free_recovery(V):
    cams = rig(V, 10 + V)
    g = np.random.Generator(np.random.PCG64(V))
    X = np.array([0.0, 0.0, 1.0]) + g.uniform(-0.6, 0.6, (8, 22, 3))
    r = MR.triangulate(exact_keypoints(cams, X), cams, as_given=True)
    assert np.abs(r['joints'] - X).max() <= 1e-9
    assert (r['report'][..., 0] == V).all() and (r['inliers'] == (1 << V) - 1).all() and (r['report'][..., 3] == V).all()
    assert np.abs(r['conf'] - 1.0).max() <= 1e-7
    # view_residuals reads float32 detections, as its kernel does: half a float32 step at 1024 px is 6.1e-5 px per coordinate
    assert np.nanmax(MR.view_residuals(r['joints'], exact_keypoints(cams, X), cams)) <= 8.7e-5


@pytest.mark.parametrize('V,seed', [(2, 0), (4, 1), (6, 2), (16, 3)])
def test_noise_stays_within_five_sigma(V, seed):
    cams = rig(V, 20 + seed)
    kp, X = MR.make_views(cams, 16, 25, 30 + seed, noise_px=2.0)
    r = MR.triangulate(kp, cams)
    err = np.linalg.norm(r['joints'] - X, axis=-1)
    assert np.isfinite(err).all()
    ratio = err / (2.0 * r['report'][..., 2])
    print(f'V = {V}: median error {np.median(err) * 1e3:.1f} mm, worst error / (2 px sigma_m) = {ratio.max():.2f}')
    assert (ratio <= 5.0).all()


@pytest.mark.parametrize('V,bad,seed', [(4, 1, 0), (6, 2, 1), (16, 5, 2)])
def test_planted_outliers_are_never_inliers(V, bad, seed):
    cams = rig(V, 40 + seed)
    kp, X = MR.make_views(cams, 16, 25, 50 + seed, noise_px=2.0)          # 400 points
    kp, planted = MR.plant_outliers(kp, bad, 60 + seed)
    r = MR.triangulate(kp, cams)
    bits = np.stack([(r['inliers'] >> v) & 1 for v in range(V)]).astype(bool)
    assert not (bits & planted).any()
    err = np.linalg.norm(r['joints'] - X, axis=-1)
    print(f'{bad} of {V} views planted: median error {np.nanmedian(err) * 1e3:.1f} mm, {int(np.isnan(err).sum())} points without a result')
    assert (r['report'][..., 0] >= 2).all() and (r['report'][..., 0] <= V - bad).all()
    assert np.nanmedian(err) <= 0.02                                       # (the prototype: 9.2 / 8.1 / 4.8 mm)


def test_no_result_rule_clause_by_clause():
    cams = rig(3, 70)
    X = np.array([0.0, 0.0, 1.0]) + np.zeros((1, 9, 3))
    kp = exact_keypoints(cams, X, conf=0.9).astype(np.float32)

    def none(r, j, n_obs):
        return (np.isnan(r['joints'][0, j]).all() and r['conf'][0, j] == 0 and r['inliers'][0, j] == 0 and r['report'][0, j, 0] == 0 and
                np.isnan(r['report'][0, j, 1:3]).all() and r['report'][0, j, 3] == n_obs)
    kp[0, 0, 0, 0], kp[1, 0, 0, 1] = np.nan, np.inf                        # joint 0: NaN x and infinite y leave one view
    kp[0, 0, 1, 2], kp[2, 0, 1, 2] = np.nan, np.inf                        # joint 1: NaN and infinite c leave one view
    kp[0, 0, 2, 2], kp[1, 0, 2, 2] = 0.25, 0.1                             # joint 2: c <= conf_min (0.25, exact in float32) leaves one view
    kp[0, 0, 3, 2] = 0.25                                                  # joint 3: two views are enough
    kp[2, 0, 4, :2] += 200.0                                               # joint 4: min_views = 3 with two inliers
    r = MR.triangulate(kp, cams, conf_min=0.25, want_undistorted=True)
    for j in (0, 1, 2):
        assert none(r, j, 1)
    assert r['report'][0, 3, 0] == 2 and r['inliers'][0, 3] == 0b110 and np.abs(r['joints'][0, 3] - X[0, 3]).max() < 1e-6
    assert r['report'][0, 4, 0] == 2 and r['inliers'][0, 4] == 0b011
    assert r['report'][0, 5, 0] == 3
    assert none(MR.triangulate(kp, cams, conf_min=0.25, min_views=3), 4, 3)
    # an unobserved entry of keypoints_und passes through as given, bit for bit; an observed one keeps its confidence
    und = r['keypoints_und']
    assert np.array_equal(und[0, 0, 0].view(np.uint32), kp[0, 0, 0].view(np.uint32)) and np.array_equal(und[..., 2].view(np.uint32), kp[..., 2].view(np.uint32))
    assert np.abs(und[2, 0, 5, :2] - kp[2, 0, 5, :2]).max() == 0           # no distortion: the same pixels
    # a point behind a camera: the pair's own view has an infinite error, so the pair is no candidate
    behind = rig(2, 71)
    Xb = (-np.linalg.inv(behind[0, :9].reshape(3, 3)) @ behind[0, 9:12])[None, None] + np.array([0.3, 0.2, 0.5])    # near camera 0's centre
    zc = behind[:, :9].reshape(2, 3, 3) @ Xb[0, 0] + behind[:, 9:12]
    kpb = exact_keypoints(behind, Xb)
    if zc[0, 2] > 0:                                                       # put it behind camera 0 whichever way that camera looks
        Xb = Xb - 2 * zc[0, 2] * behind[0, 6:9]
        kpb = exact_keypoints(behind, Xb)
    assert (behind[0, 6:9] @ Xb[0, 0] + behind[0, 11]) < 0
    rb = MR.triangulate(kpb, behind, as_given=True)
    assert np.isnan(rb['joints']).all() and rb['report'][0, 0, 3] == 2 and rb['report'][0, 0, 0] == 0
    assert np.isnan(MR.view_residuals(Xb, kpb, behind)[0]).all() and np.isfinite(MR.view_residuals(Xb, kpb, behind)[1]).all()
    # two identical cameras: parallel rays propose nothing
    twin = np.stack([cams[0], cams[0]])
    rt = MR.triangulate(np.stack([kp[0], kp[0]])[:, :, 5:6], twin)
    assert np.isnan(rt['joints']).all() and rt['report'][0, 0, 3] == 2 and rt['report'][0, 0, 0] == 0


def test_refinement_never_raises_the_cost_and_keeps_the_start_when_told():
    cams = rig(5, 80, distortion=True)
    kp, _ = MR.make_views(cams, 4, 22, 81, noise_px=2.0)
    r0, r3 = MR.triangulate(kp, cams, refine=0), MR.triangulate(kp, cams, refine=3)
    assert np.array_equal(r0['inliers'], r3['inliers'])
    assert (r3['report'][..., 1] <= r0['report'][..., 1]).all() and (r3['report'][..., 1] < r0['report'][..., 1]).any()


# ---- the host logic --------------------------------------------------------------------------------------------------------------
def views_file(V=4, N=5, K=25, seed=90, distortion=True, **extra):
    Kc, W, D = MR.make_rig(V, seed, distortion)
    cams = multiview.pack_cameras(Kc, W, D)
    kp, X = MR.make_views(cams, N, K, seed + 1, noise_px=0.0)
    d = {'keypoints_2d': kp, 'camera_mtx': Kc, 'world2cam': W, 'fps': 30.0}
    if D is not None:
        d['dist_coeffs'] = D
    d.update(extra)
    return d, X


def test_pack_cameras_layout():
    Kc, W, D = MR.make_rig(3, 1, True)
    cams = multiview.pack_cameras(Kc, W, D)
    assert cams.shape == (3, 24) and cams.dtype == np.float64
    assert np.array_equal(cams[:, :9].reshape(3, 3, 3), W[:, :3, :3]) and np.array_equal(cams[:, 9:12], W[:, :3, 3])
    assert np.array_equal(cams[:, 12:16], np.stack([Kc[:, 0, 0], Kc[:, 1, 1], Kc[:, 0, 2], Kc[:, 1, 2]], 1))
    assert np.array_equal(cams[:, 16:21], D) and not cams[:, 21:].any()
    assert not multiview.pack_cameras(Kc, W)[:, 16:].any()
    skew = Kc.copy()
    skew[1, 0, 1] = 0.5
    with pytest.raises(ValueError, match='skew'):
        multiview.pack_cameras(skew, W)


def test_read_views_refusals():
    d, _ = views_file()
    v = multiview.read_views(d)
    assert v['keypoints'].shape == (4, 5, 25, 3) and v['time_key'] == 'fps'
    c2w = dict(d, cam2world=np.linalg.inv(d['world2cam']))
    del c2w['world2cam']
    assert np.abs(multiview.read_views(c2w)['world2cam'] - d['world2cam']).max() < 1e-12
    with pytest.raises(ValueError, match=r"unknown keys \['depth_maps'\]"):
        multiview.read_views(dict(d, depth_maps=np.zeros(3)))
    with pytest.raises(ValueError, match='exactly one of world2cam and cam2world'):
        multiview.read_views(dict(d, cam2world=d['world2cam']))
    with pytest.raises(ValueError, match='exactly one of world2cam and cam2world'):
        multiview.read_views({k: x for k, x in d.items() if k != 'world2cam'})
    with pytest.raises(ValueError, match='exactly one of fps and times'):
        multiview.read_views(dict(d, times=np.arange(5) / 30.0))
    with pytest.raises(ValueError, match='exactly one of fps and times'):
        multiview.read_views({k: x for k, x in d.items() if k != 'fps'})
    one = {k: (x[:1] if isinstance(x, np.ndarray) else x) for k, x in d.items()}
    with pytest.raises(ValueError, match=r'views must be in \[2, 16\], got 1'):
        multiview.read_views(one)
    many = {k: (np.concatenate([x] * 5)[:17] if isinstance(x, np.ndarray) else x) for k, x in d.items()}
    with pytest.raises(ValueError, match=r'views must be in \[2, 16\], got 17'):
        multiview.read_views(many)
    with pytest.raises(ValueError, match='keypoints_2d must be'):
        multiview.read_views(dict(d, keypoints_2d=d['keypoints_2d'][:, :, :21]))
    with pytest.raises(ValueError, match='camera_mtx must be'):
        multiview.read_views(dict(d, camera_mtx=d['camera_mtx'][:3]))
    with pytest.raises(ValueError, match='world2cam must be'):
        multiview.read_views(dict(d, world2cam=d['world2cam'][:, :3]))
    with pytest.raises(ValueError, match='dist_coeffs must be'):
        multiview.read_views(dict(d, dist_coeffs=d['dist_coeffs'][:, :4]))
    with pytest.raises(ValueError, match='times must be'):
        multiview.read_views(dict({k: x for k, x in d.items() if k != 'fps'}, times=np.arange(4) / 30.0))
    with pytest.raises(ValueError, match='world_up_axis'):
        multiview.read_views(dict(d, world_up_axis='x'))
    with pytest.raises(ValueError, match='frame_names must be'):
        multiview.read_views(dict(d, frame_names=np.array(['a', 'b'])))
    with pytest.raises(ValueError, match='missing'):
        multiview.read_views({k: x for k, x in d.items() if k != 'camera_mtx'})


@pytest.fixture()
def on_reference(monkeypatch):
    monkeypatch.setattr(multiview, 'triangulate', MR.torch_triangulate)
    monkeypatch.setattr(multiview, 'view_residuals', MR.torch_view_residuals)


@pytest.mark.parametrize('K', [22, 25])
def test_triangulate_views_gives_a_skeleton_file(on_reference, K, tmp_path):
    d, X = views_file(K=K, world_up_axis='z', floor_height=0.0, recording_name='rig', frame_names=np.array(['f%d' % i for i in range(5)]))
    d['keypoints_2d'] = d['keypoints_2d'].copy()
    d['keypoints_2d'][:, 2, 7, 2] = 0.0                                    # one point nobody sees
    path = tmp_path / 'views.npz'
    np.savez(path, **d)
    skeleton, summary = multiview.triangulate_views(str(path), ref_view=1, device='cpu')
    assert set(skeleton) <= set(fit.SKELETON_KEYS) | set(fit.PASS_THROUGH)
    assert set(skeleton) == {'joints_3d', 'joint_conf', 'fps', 'keypoints_2d', 'focal_length', 'camera_center', 'cam2world', 'up_axis', 'floor_height',
                             'frame_names', 'recording_name'}
    joints, conf, betas, times, extra = fit.read_skeleton(skeleton)
    assert joints.shape == (5, 22, 3) and conf.shape == (5, 22) and betas is None and np.allclose(times, np.arange(5) / 30.0)
    W = d['world2cam'][1]
    want = X @ W[:3, :3].T + W[:3, 3]
    got = skeleton['joints_3d']
    assert got.shape == (5, K, 3) and got.dtype == np.float32
    seen = np.ones((5, K), bool)
    seen[2, 7] = False
    assert np.isnan(got[2, 7]).all() and skeleton['joint_conf'][2, 7] == 0
    assert np.abs(got[seen] - want[seen]).max() < 1e-5                     # float32 pixels and joints
    assert np.abs(skeleton['cam2world'] @ W - np.eye(4)).max() < 1e-12
    assert skeleton['keypoints_2d'].shape == (5, K, 3)
    assert list(skeleton['focal_length']) == [d['camera_mtx'][1, 0, 0], d['camera_mtx'][1, 1, 1]]
    # the undistorted keypoints are the pinhole projection of the joints in the reference view
    pin = want[..., :2] / want[..., 2:] * skeleton['focal_length'] + skeleton['camera_center']
    assert np.abs(skeleton['keypoints_2d'][..., :2][seen] - pin[seen]).max() < 1e-3
    assert summary['triangulated'] == 5 * K - 1 and summary['without_result'] == 1 and summary['inlier_histogram'] == {'0': 1, '4': 5 * K - 1}
    assert len(summary['per_view']) == 4 and all(r['rejected_share'] == 0.0 and r['residual_p95_px'] < 1e-3 for r in summary['per_view'])
    assert 0 < summary['median_sigma_m'] < 0.01
    # without world_up_axis nothing about the world is handed on: rohm_amd.floor finds it
    bare, _ = multiview.triangulate_views({k: x for k, x in d.items() if k not in ('world_up_axis', 'floor_height')}, device='cpu')
    assert not {'cam2world', 'up_axis', 'floor_height'} & set(bare)
    with pytest.raises(ValueError, match='ref_view'):
        multiview.triangulate_views(d, ref_view=4, device='cpu')


def test_the_kernels_refuse_cpu_tensors():
    cams = torch.from_numpy(rig(2, 1))
    kp = torch.zeros(2, 1, 22, 3)
    with pytest.raises(Exception, match='no CPU fallback'):
        multiview.triangulate(kp, cams)
    with pytest.raises(Exception, match='no CPU fallback'):
        multiview.view_residuals(torch.zeros(1, 22, 3, dtype=torch.float64), kp, cams)


def test_margins_of_the_gpu_inputs():
    """The condition the equalities of tests/test_gpu_multiview.py rest on: no scored error within 1e-6 px of tau_px, no pair within
    1e-9 of the angle threshold, no cost gap below 1e-9 relative among the candidates at the winning count."""
    for name in MR.GPU_CASES:
        case = MR.build_case(name)
        bad = MR.margins_ok(case['ref'])
        assert len(bad) == 0, f'{name}: points {bad[:5].tolist()} are within the margins; replace the seed in GPU_CASES with a comment'
        counts = case['ref']['report'][..., 0]
        print(name, 'inlier counts', np.bincount(counts.astype(int).ravel()).tolist(), 'least margins', case['ref']['margin_tau'].min(),
              case['ref']['margin_angle'].min(), case['ref']['margin_cost'].min())


def test_argument_errors_name_the_argument():
    """The checks come before any launch and touch no pointer, so they run without a GPU."""
    import ctypes as C
    from rohm_amd import _lib
    L = _lib.lib()
    assert multiview.limits() == (16, 120)
    assert L.rohm_mv_limits(None, None) == 0

    def tri(V=4, N=1, J=22, conf_min=0.2, tau=10.0, ang=0.03, min_views=2, refine=3, kp=8, cams=8, joints=8, conf=8, report=8, inl=8):
        return L.rohm_mv_triangulate(kp, cams, None, V, N, J, conf_min, tau, ang, min_views, refine, joints, conf, report, inl, None, None)

    def res(V=4, N=1, J=22, conf_min=0.2, jw=8, kp=8, cams=8, out=8):
        return L.rohm_mv_residuals(jw, kp, cams, V, N, J, conf_min, out, None)
    for call, word in ((lambda: tri(V=1), 'V must be'), (lambda: tri(V=17), 'V must be'), (lambda: tri(N=-1), 'N must be'), (lambda: tri(J=0), 'J must be'),
                       (lambda: tri(N=1 << 20, J=1 << 10), 'N * J'), (lambda: tri(conf_min=float('nan')), 'conf_min'), (lambda: tri(tau=0.0), 'tau_px'),
                       (lambda: tri(tau=float('inf')), 'tau_px'), (lambda: tri(ang=-0.1), 'min_angle_rad'), (lambda: tri(ang=float('nan')), 'min_angle_rad'),
                       (lambda: tri(min_views=1), 'min_views'), (lambda: tri(min_views=5), 'min_views'), (lambda: tri(refine=-1), 'refine'),
                       (lambda: tri(refine=65), 'refine'), (lambda: tri(kp=None), 'keypoints'), (lambda: tri(cams=None), 'cams'),
                       (lambda: tri(joints=None), 'joints'), (lambda: tri(conf=None), 'conf is null'), (lambda: tri(report=None), 'report'),
                       (lambda: tri(inl=None), 'inliers'), (lambda: res(V=1), 'V must be'), (lambda: res(N=-1), 'N must be'),
                       (lambda: res(jw=None), 'joints_world'), (lambda: res(kp=None), 'keypoints'), (lambda: res(cams=None), 'cams'),
                       (lambda: res(out=None), 'resid')):
        assert call() == -1
        assert word in L.rohm_last_error().decode()
    # N == 0 returns without a launch, whatever the pointers
    assert tri(N=0, kp=None, cams=None, joints=None, conf=None, report=None, inl=None) == 0 and res(N=0, jw=None, kp=None, cams=None, out=None) == 0
