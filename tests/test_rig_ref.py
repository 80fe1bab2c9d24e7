"""CPU: the float64 restatement of the rig calibration (tests/rig_ref.py, the rule of include/rohm_rig.h) held to closed forms,
central differences, a stacked dense Jacobian and the recovery of planted rigs; `rohm_amd.rig`'s host logic run on the
restatement; and the margins the equalities of tests/test_gpu_rig.py rest on.

Recovery bars.  Four planted scenes -- (V, N, noise px, outlier share) = (4, 60, 2, 0), (4, 60, 2, 0.1), (6, 30, 2, 0.2), (3, 20, 1,
0.05), `multiview_ref.make_rig` cameras with distortion 4 m away, a 22-point body that walks a 1.2 m circle, 256 hypotheses per
pair -- were run once with the restatement; the worst rotation / camera-centre errors after bundle adjustment were 0.026 deg / 3.3 mm,
0.063 / 3.5, 0.073 / 3.9 and 0.039 / 2.9 (profiles/rig_parity.json, group `recovery`).  The bars RECOVERY_BARS are twice those, rounded
up: the factor of two is for seed-to-seed spread.  The median residual after bundle adjustment must be within 1.25 x the noise (at
the optimum it is below the noise; 25 % covers the robust kernel's bias), and bundle adjustment must lower both errors."""
import functools

import numpy as np
import pytest
import torch

import fit_ref as FR
import multiview_ref as MR
import rig_ref as RR
from rohm_amd import multiview, rig
from rohm_amd.utils import synth

record = RR.record
RECOVERY, RECOVERY_BARS = RR.RECOVERY, RR.RECOVERY_BARS
_RUNS = {}
calibrate_views = functools.partial(rig.calibrate_views, device='cpu')


@pytest.fixture()
def on_reference(monkeypatch):
    RR.on_reference(monkeypatch)


def two_cameras(seed, n=8):
    """(I | 0) and (R | t) with unit intrinsics-free pixels: cams [2,24], keypoints [2,1,n,3] float64 (exact), R, t."""
    g = np.random.Generator(np.random.PCG64(seed))
    R = RR.rodrigues(g.standard_normal(3) * 0.4)
    t = g.standard_normal(3)
    t /= np.linalg.norm(t)
    X = g.uniform(-1.0, 1.0, (n, 3)) * np.array([2.0, 2.0, 2.0]) + np.array([0.0, 0.0, 5.0])      # a deep, wide cloud: a well-conditioned M
    cams = np.zeros((2, 24))
    cams[0, :9], cams[1, :9], cams[1, 9:12] = np.eye(3).reshape(9), R.reshape(9), t
    cams[:, 12], cams[:, 13], cams[:, 14], cams[:, 15] = (900.0, 1100.0), (950.0, 1050.0), 640.0, 360.0
    kp = np.ones((2, 1, n, 3))
    for v in range(2):
        xc = X @ cams[v, :9].reshape(3, 3).T + cams[v, 9:12]
        kp[v, 0, :, 0] = cams[v, 12] * xc[:, 0] / xc[:, 2] + cams[v, 14]
        kp[v, 0, :, 1] = cams[v, 13] * xc[:, 1] / xc[:, 2] + cams[v, 15]
    return cams, kp, R, t


# ---- 1: the eight-point rule -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', [1, 7, 20])                           # clouds whose eigen-gap is above the GPU tests' margin
def test_eight_exact_points_give_back_the_essential_matrix(seed):
    cams, kp, R, t = two_cameras(seed)
    res = RR.pair_hypotheses(kp, cams, [[0, 1]], np.arange(8, dtype=np.int32).reshape(1, 1, 8), as_given=True)
    want = (RR.cross_matrix(t) @ R).reshape(9)
    want, _ = RR.fix_sign(want / np.linalg.norm(want))
    assert res['gap'][0, 0] > 1e-6                                         # the GPU tests' margin: the eigenvector is good to 1e-16 / 1e-6
    assert np.abs(res['E'][0, 0] - want).max() <= 1e-9
    assert res['counts'][0, 0].tolist() == [8, 8] and res['best'][0] == 0
    ab = RR.undistorted(kp, cams, as_given=True)
    assert RR.sampson(want, ab[0], ab[1], RR.pair_scale(cams, 0, 1)).max() <= 1e-9
    assert np.argmax(np.abs(res['E'][0, 0])) == np.argmax(res['E'][0, 0])              # the sign rule


# ---- 2: the degeneracy clauses, one by one ---------------------------------------------------------------------------------------------
def test_every_degeneracy_clause():
    cams, kp, _, _ = two_cameras(4, n=12)
    kp[1, 0, 11, 2] = 0.0                                                  # point 11 is not seen by view 1
    base = np.arange(8, dtype=np.int32)

    def run(samples, pairs=((0, 1),)):
        return RR.pair_hypotheses(kp, cams, np.array(pairs), np.array(samples, dtype=np.int32).reshape(len(pairs), -1, 8), as_given=True)

    def dead(res, q=0, k=0):
        return np.isnan(res['E'][q, k]).all() and res['counts'][q, k].tolist() == [-1, -1]
    ok = run([base])
    assert not dead(ok) and ok['counts'][0, 0, 1] == 11 and ok['best'][0] == 0
    for pair in ((0, 2), (-1, 1), (1, 1)):                                 # a pair entry outside [0, V), or v1 = v2
        r = run([base], (pair,))
        assert dead(r) and r['best'][0] == -1
    for bad in (12, -1):                                                   # a sample index outside [0, N J)
        s = base.copy()
        s[3] = bad
        assert dead(run([s]))
    s = base.copy()
    s[6] = s[2]                                                            # repeated
    assert dead(run([s]))
    s = base.copy()
    s[0] = 11                                                              # not common to both views
    assert dead(run([s]))
    flat = kp.copy()                                                       # eight points whose rows span only seven dimensions: lambda_2 = 0
    flat[:, 0, 1:8, :2] = flat[:, 0, :1, :2] + np.arange(1, 8)[None, :, None] * np.array([3.0, 0.0])      # both views see the same line
    r = RR.pair_hypotheses(flat, cams, [[0, 1]], base.reshape(1, 1, 8), as_given=True)
    assert dead(r)
    # a degenerate hypothesis never wins; the lowest index wins a tie
    r = run([[12] * 8, base, base])
    assert dead(r, 0, 0) and r['best'][0] == 1 and r['counts'][0, 1].tolist() == r['counts'][0, 2].tolist()


# ---- 3: Jacobians and gradient -----------------------------------------------------------------------------------------------------------
def test_jacobians_match_central_differences():
    g = np.random.Generator(np.random.PCG64(5))
    cams = multiview.pack_cameras(*MR.make_rig(3, 11, True))
    X = np.array([0.2, -0.1, 1.1])
    a, b = 0.05, -0.02
    h = 1e-6
    for v in range(3):
        r0, JX, Jc, zc = RR.ba_terms(cams[v], X, a, b)
        assert zc > 0
        for k in range(3):
            d = np.zeros(3)
            d[k] = h
            num = (RR.ba_terms(cams[v], X + d, a, b)[0] - RR.ba_terms(cams[v], X - d, a, b)[0]) / (2 * h)
            assert np.abs(num - JX[:, k]).max() <= 1e-6 * np.abs(JX).max()
        for k in range(6):
            d = np.zeros(6)
            d[k] = h
            rs = []
            for sgn in (1.0, -1.0):
                c = cams[v].copy()
                c[:9] = (RR.rodrigues(sgn * d[:3]) @ cams[v, :9].reshape(3, 3)).reshape(9)
                c[9:12] += sgn * d[3:]
                rs.append(RR.ba_terms(c, X, a, b)[0])
            assert np.abs((rs[0] - rs[1]) / (2 * h) - Jc[:, k]).max() <= 1e-6 * np.abs(Jc).max()


@pytest.mark.parametrize('sigma_px', [0.0, 10.0])
def test_gradient_of_half_the_energy(sigma_px):
    case = RR.build_ba_case('three_views')
    kp, cams, X = case['keypoints'], np.array(case['cams']), np.array(case['points'])
    t = RR.ba_normal(kp, cams, X, sigma_px=sigma_px)
    h = 1e-6
    ins = np.flatnonzero(t['inside'])
    assert len(ins) > 10 and (~t['inside']).any()
    for p in ins[:4]:
        for k in range(3):
            Xp, Xm = X.copy(), X.copy()
            Xp[p, k] += h
            Xm[p, k] -= h
            num = (RR.ba_energy(kp, cams, Xp, sigma_px=sigma_px) - RR.ba_energy(kp, cams, Xm, sigma_px=sigma_px)) / (4 * h)
            assert abs(num - t['gp'][p, k]) <= 1e-5 * max(1.0, np.abs(t['gp'][p]).max())
    for v in range(3):
        for k in range(6):
            Es = []
            for sgn in (1.0, -1.0):
                dc = np.zeros((3, 6))
                dc[v, k] = sgn * h
                Es.append(RR.ba_energy(kp, RR.ba_update(kp, cams, X, dc)[1], X, sigma_px=sigma_px))
            assert abs((Es[0] - Es[1]) / (4 * h) - t['gc'][v, k]) <= 1e-5 * max(1.0, np.abs(t['gc'][v]).max())


# ---- 4: the reduced system against the stacked dense Jacobian -----------------------------------------------------------------------------
@pytest.mark.parametrize('sigma_px,lam', [(0.0, 1e-3), (10.0, 1e2)])
def test_reduced_system_equals_the_dense_one(sigma_px, lam):
    V, P = 3, 5
    cams = multiview.pack_cameras(*MR.make_rig(V, 21, True))
    kp, X = MR.make_views(cams, 1, P, 22, noise_px=2.0)
    kp[1, 0, 2, 2] = 0.0                                                   # one unobserved entry
    X = X.reshape(P, 3) + 0.01
    ab, c, obs, inside, _ = RR.ba_problem(kp, cams, X)
    rows, res = [], []
    for p in range(P):
        for v in np.flatnonzero(obs[:, p]):
            r, JX, Jc, _ = RR.ba_terms(cams[v], X[p], ab[v, p, 0], ab[v, p, 1])
            w = c[v, p] * RR.rho(np.float64(r @ r), sigma_px)[1]
            J = np.zeros((2, 6 * V + 3 * P))
            J[:, 6 * v:6 * v + 6], J[:, 6 * V + 3 * p:6 * V + 3 * p + 3] = Jc, JX
            rows.append(np.sqrt(w) * J)
            res.append(np.sqrt(w) * r)
    J, res = np.concatenate(rows), np.concatenate(res)
    H, g = J.T @ J, J.T @ res
    Hd = H + lam * np.diag(np.diag(H) + 1e-9)
    n = 6 * V
    Hpp_inv = np.linalg.inv(Hd[n:, n:])
    S = Hd[:n, :n] - Hd[:n, n:] @ Hpp_inv @ Hd[n:, :n]
    rr = g[:n] - Hd[:n, n:] @ Hpp_inv @ g[n:]
    got = RR.ba_moments(kp, cams, X, sigma_px=sigma_px, lam=lam)
    assert got['n_obs'] == int(obs.sum()) == V * P - 1
    assert np.abs(got['S'] - S).max() <= 1e-9 * np.abs(S).max() and np.abs(got['r'] - rr).max() <= 1e-9 * np.abs(rr).max()
    full = -np.linalg.solve(Hd, g)
    dc = -np.linalg.solve(got['S'], got['r'])
    assert np.abs(dc - full[:n]).max() <= 1e-9 * np.abs(full[:n]).max()
    Xn, cn = RR.ba_update(kp, cams, X, dc.reshape(V, 6), sigma_px=sigma_px, lam=lam)
    assert np.abs(Xn - (X + full[n:].reshape(P, 3))).max() <= 1e-9 * np.abs(X).max()
    assert np.abs(cn[:, 9:12] - cams[:, 9:12] - dc.reshape(V, 6)[:, 3:]).max() <= 1e-15 and np.array_equal(cn[:, 12:], cams[:, 12:])


def test_a_point_behind_a_camera_gives_an_infinite_energy():
    case = RR.build_ba_case('three_views')
    X = np.array(case['points'])
    p = int(np.flatnonzero(RR.ba_problem(case['keypoints'], case['cams'], X)[3])[0])
    C = -case['cams'][0, :9].reshape(3, 3).T @ case['cams'][0, 9:12]
    X[p] = C - case['cams'][0, 6:9]                                        # a metre behind camera 0
    m = RR.ba_moments(case['keypoints'], case['cams'], X)
    assert m['E'] == np.inf and np.isfinite(m['S']).all() and np.isfinite(m['r']).all()


# ---- 5 and 6: recovery ----------------------------------------------------------------------------------------------------------------------
def recovery_run(name, monkeypatch):
    if name not in _RUNS:
        RR.on_reference(monkeypatch)
        V, N, noise, share, seed = RECOVERY[name]
        K, W, D, kp, X = RR.make_scene(V, N, 22, seed, noise, share)
        w2c, rep = rig.calibrate(kp, K, D, hypotheses=256, device='cpu')
        _RUNS[name] = (W, w2c, rep, noise)
    return _RUNS[name]


@pytest.mark.parametrize('name', list(RECOVERY))
def test_planted_rig_is_recovered(name, monkeypatch):
    W, w2c, rep, noise = recovery_run(name, monkeypatch)
    nb = rep['neighbour']
    rot0, ctr0 = RR.rig_errors(rep['chained_world2cam'], W, 0, nb)
    rot, ctr = RR.rig_errors(w2c, W, 0, nb)
    print(f'{name}: chained {rot0:.3f} deg / {1e3 * ctr0:.1f} mm, adjusted {rot:.3f} deg / {1e3 * ctr:.1f} mm, median residual '
          f'{rep["median_residual_px"]:.2f} px, {rep["iterations"]} iterations')
    record('recovery', name + '_chained_rotation_deg', rot0)
    record('recovery', name + '_chained_centre_m', ctr0)
    record('recovery', name + '_rotation_deg', rot)
    record('recovery', name + '_centre_m', ctr)
    record('recovery', name + '_median_residual_px', rep['median_residual_px'])
    assert rot <= RECOVERY_BARS[name][0] and ctr <= RECOVERY_BARS[name][1]
    assert rep['median_residual_px'] <= 1.25 * noise
    assert rot < rot0 and ctr < ctr0                                       # bundle adjustment lowers both
    assert abs(np.linalg.norm(w2c[nb, :3, :3].T @ w2c[nb, :3, 3]) - 1.0) < 1e-12 and np.array_equal(w2c[0], np.eye(4))


@pytest.mark.parametrize('name', list(RECOVERY))
def test_energy_never_rises(name, monkeypatch):
    rep = recovery_run(name, monkeypatch)[2]
    E = np.array(rep['energy'])
    assert len(E) == rep['iterations'] + 1 >= 3 and np.isfinite(E).all() and (np.diff(E) <= 0).all() and E[-1] < E[0]


# ---- 7: scale --------------------------------------------------------------------------------------------------------------------------
def body_views(V=4, N=12, seed=71, K=22):
    """A views file without extrinsics: the synthetic body, noise-free, seen by V distorting cameras -> (dict, world2cam)."""
    clean = FR.make_frames(synth.synthetic_smplx_tensors(0), N, seed=seed, pose_scale=0.12, root_angle=0.5, centre=(0.0, 0.0, 1.0))[0].astype(np.float64)
    Kc, W, D = MR.make_rig(V, seed + 1, True)
    px, depth = MR.project(multiview.pack_cameras(Kc, W, D), clean.reshape(-1, 3))
    assert (depth > 1.0).all()
    kp = np.concatenate([px, np.ones(px.shape[:2] + (1,))], -1).reshape(V, N, 22, 3).astype(np.float32)
    if K == 25:
        from rohm_amd.data_loaders.dataloader_video import OPENPOSE_TO_SMPL
        body25 = np.zeros((V, N, 25, 3), np.float32)
        for smpl, op in enumerate(OPENPOSE_TO_SMPL[:22]):
            if smpl not in (3, 6, 9, 13, 14, 10, 11):                     # the joints BODY_25 has a true counterpart for (and the feet, unused)
                body25[:, :, op] = kp[:, :, smpl]
        kp = body25
    return {'keypoints_2d': kp, 'camera_mtx': Kc, 'dist_coeffs': D, 'fps': 30.0, 'recording_name': np.array('rig')}, W


@pytest.mark.parametrize('K', [22, 25])
def test_bones_and_baseline_scale(on_reference, K):
    from rohm_amd.body_model import SMPLXLayer
    d, W = body_views(K=K)
    layer = SMPLXLayer.from_tensors(synth.synthetic_smplx_tensors(0))
    out, rep = calibrate_views(d, body_model=layer, hypotheses=64, iters=10, min_inliers=30)
    assert rep['scale_from'] == 'bones'
    nb = rep['neighbour']
    true = np.linalg.norm((W @ np.linalg.inv(W[0]))[nb, :3, 3])
    got = np.linalg.norm(out['world2cam'][nb, :3, 3])
    print(f'K = {K}: bones scale {got:.5f} m against the true baseline {true:.5f} m')
    record('recovery', 'bones_scale_rel', abs(got / true - 1.0))
    assert abs(got / true - 1.0) <= 0.01
    out, rep = calibrate_views(d, scale_from='baseline', baseline_m=2.5, hypotheses=64, iters=10, min_inliers=30)
    assert abs(np.linalg.norm(out['world2cam'][rep['neighbour'], :3, 3]) - 2.5) < 1e-12
    out, rep = calibrate_views(d, hypotheses=64, iters=10, min_inliers=30)
    assert rep['scale_from'] == 'none' and abs(np.linalg.norm(out['world2cam'][rep['neighbour'], :3, 3]) - 1.0) < 1e-12


# ---- 8: the views file, the refusals, the argument errors, the table ---------------------------------------------------------------------
def test_calibrate_views_fills_in_world2cam(on_reference, tmp_path):
    d, W = body_views()
    d['frame_names'] = np.array(['f%d' % i for i in range(12)])
    path = tmp_path / 'uncalibrated.npz'
    np.savez(path, **d)
    out, rep = calibrate_views(str(path), hypotheses=64, iters=10, min_inliers=30, ref_view=1)
    assert set(out) == set(d) | {'world2cam'} and 'world_up_axis' not in out
    v = multiview.read_views(out)                                          # the output is a views file as it stands
    assert v['keypoints'].shape == (4, 12, 22, 3) and np.array_equal(out['world2cam'][1], np.eye(4))
    rot, ctr = RR.rig_errors(out['world2cam'], W, 1, rep['neighbour'])
    assert rot < 0.01 and ctr < 1e-3                                       # noise-free
    assert len(rep['pairs']) == 6 and all(p['inlier_share'] > 0.9 for p in rep['pairs']) and len(rep['tree']) == 3
    assert all(r['residual_median_px'] < 0.05 for r in rep['per_view'])
    assert rig.main(['--views', str(path), '--out', str(tmp_path / 'views.npz'), '--json', str(tmp_path / 'report.json'), '--hypotheses', '64',
                     '--iters', '5', '--min_inliers', '30', '--device', 'cpu']) == 0
    assert multiview.read_views(str(tmp_path / 'views.npz'))['world2cam'].shape == (4, 4, 4)
    import json
    with open(tmp_path / 'report.json') as f:
        js = json.load(f)
    assert js['report']['iterations'] >= 1 and len(js['report']['energy']) == js['report']['iterations'] + 1 and js['options']['hypotheses'] == 64


def test_refusals_name_the_cause(on_reference):
    d, _ = body_views()
    with pytest.raises(ValueError, match='calibrated already'):
        calibrate_views(dict(d, world2cam=np.broadcast_to(np.eye(4), (4, 4, 4))))
    with pytest.raises(ValueError, match=r"unknown keys \['depth_maps'\]"):
        calibrate_views(dict(d, depth_maps=np.zeros(3)))
    with pytest.raises(ValueError, match='camera_mtx must be'):
        calibrate_views(dict(d, camera_mtx=d['camera_mtx'][:3]))
    with pytest.raises(ValueError, match='world_up_axis'):
        calibrate_views(dict(d, world_up_axis='z'))
    with pytest.raises(ValueError, match='bones needs a body model'):
        calibrate_views(d, scale_from='bones')
    with pytest.raises(ValueError, match='baseline_m'):
        calibrate_views(d, scale_from='baseline')
    with pytest.raises(ValueError, match='scale_from must be'):
        calibrate_views(d, scale_from='metres')
    blind = dict(d, keypoints_2d=d['keypoints_2d'].copy())
    blind['keypoints_2d'][..., 2] = 0.0
    with pytest.raises(ValueError, match='no common points'):
        calibrate_views(blind)
    lone = dict(d, keypoints_2d=d['keypoints_2d'].copy())
    lone['keypoints_2d'][2, 1:, :, 2] = 0.0                                # view 2 sees one frame: 22 common points with anyone
    with pytest.raises(ValueError, match='view 2: every pair with it has fewer than min_inliers = 30'):
        calibrate_views(lone, hypotheses=32, min_inliers=30)
    with pytest.raises(ValueError, match='ref_view'):
        calibrate_views(d, ref_view=4)
    with pytest.raises(ValueError, match='min_inliers >= 8'):
        calibrate_views(d, min_inliers=7)


def test_the_kernels_refuse_cpu_tensors():
    kp, cams = torch.zeros(2, 1, 22, 3), torch.zeros(2, 24, dtype=torch.float64)
    pairs, samples = torch.zeros(1, 2, dtype=torch.int32), torch.zeros(1, 1, 8, dtype=torch.int32)
    for call in (lambda: rig.pair_hypotheses(kp, cams, pairs, samples), lambda: rig.pair_moments(kp, cams, pairs, torch.zeros(1, 9, dtype=torch.float64)),
                 lambda: rig.ba_moments(kp, cams, torch.zeros(22, 3, dtype=torch.float64)),
                 lambda: rig.ba_update(kp, cams, torch.zeros(22, 3, dtype=torch.float64), torch.zeros(2, 6, dtype=torch.float64))):
        with pytest.raises(Exception, match='no CPU fallback'):
            call()


def test_argument_errors_name_the_argument():
    """The checks come before any launch and touch no pointer, so they run without a GPU."""
    from rohm_amd import _lib
    L = _lib.lib()
    assert rig.pair_ws_bytes(4, 1750) == 4 * 1750 * 16
    assert rig.ba_ws_bytes(4, 1750) == 110 * (6 * 10 * 6 + 24 + 29 * 4) * 8         # 110 tiles of 16, one per workgroup
    assert rig.ba_ws_bytes(3, 4400) == 138 * (6 * 6 * 6 + 18 + 29 * 3) * 8          # 275 tiles, two per workgroup
    assert L.rohm_rig_pair_ws_bytes(1, 10) == -1 and 'V must be' in L.rohm_last_error().decode()
    assert L.rohm_rig_ba_ws_bytes(4, 0) == -1 and 'P must be' in L.rohm_last_error().decode()

    def hyp(V=4, N=1, J=22, Q=1, K=4, conf_min=0.2, tau=4.0, kp=8, cams=8, pairs=8, samples=8, ws=8, E=8, counts=8, best=8):
        return L.rohm_rig_pair_hypotheses(kp, cams, pairs, samples, V, N, J, Q, K, conf_min, tau, ws, E, counts, best, None)

    def mom(V=4, N=1, J=22, Q=1, conf_min=0.2, tau=4.0, kp=8, cams=8, pairs=8, E=8, ws=8, out=8):
        return L.rohm_rig_pair_moments(kp, cams, pairs, E, V, N, J, Q, conf_min, tau, ws, out, None)

    def bam(V=4, N=1, J=22, conf_min=0.2, sigma=10.0, lam=1e-3, kp=8, cams=8, pts=8, ws=8, S=8, r=8, stats=8):
        return L.rohm_rig_ba_moments(kp, cams, pts, V, N, J, conf_min, sigma, lam, ws, S, r, stats, None)

    def bau(V=4, N=1, J=22, conf_min=0.2, sigma=10.0, lam=1e-3, kp=8, cams=8, pts=8, dc=8, out=8):
        return L.rohm_rig_ba_update(kp, cams, pts, dc, V, N, J, conf_min, sigma, lam, out, None, None)
    nan, inf = float('nan'), float('inf')
    for call, word in ((lambda: hyp(V=1), 'V must be'), (lambda: hyp(V=17), 'V must be'), (lambda: hyp(N=0), 'N must be'), (lambda: hyp(J=0), 'J must be'),
                       (lambda: hyp(N=1 << 20, J=1 << 10), 'N * J'), (lambda: hyp(Q=-1), 'Q must be'), (lambda: hyp(K=0), 'K must be'),
                       (lambda: hyp(Q=1 << 14, K=1 << 14), 'Q * K'), (lambda: hyp(conf_min=nan), 'conf_min'), (lambda: hyp(tau=0.0), 'tau_px'),
                       (lambda: hyp(tau=inf), 'tau_px'), (lambda: hyp(kp=None), 'keypoints'), (lambda: hyp(cams=None), 'cams'),
                       (lambda: hyp(pairs=None), 'pairs'), (lambda: hyp(samples=None), 'samples'), (lambda: hyp(ws=None), 'ws is null'),
                       (lambda: hyp(E=None), 'E is null'), (lambda: hyp(counts=None), 'counts'), (lambda: hyp(best=None), 'best'),
                       (lambda: mom(V=1), 'V must be'), (lambda: mom(N=0), 'N must be'), (lambda: mom(Q=-1), 'Q must be'), (lambda: mom(tau=nan), 'tau_px'),
                       (lambda: mom(kp=None), 'keypoints'), (lambda: mom(cams=None), 'cams'), (lambda: mom(pairs=None), 'pairs'),
                       (lambda: mom(E=None), 'E is null'), (lambda: mom(ws=None), 'ws is null'), (lambda: mom(out=None), 'moments'),
                       (lambda: bam(V=17), 'V must be'), (lambda: bam(N=0), 'N must be'), (lambda: bam(conf_min=inf), 'conf_min'),
                       (lambda: bam(sigma=-1.0), 'sigma_px'), (lambda: bam(sigma=nan), 'sigma_px'), (lambda: bam(lam=-1.0), 'lambda'),
                       (lambda: bam(lam=inf), 'lambda'), (lambda: bam(kp=None), 'keypoints'), (lambda: bam(cams=None), 'cams'),
                       (lambda: bam(pts=None), 'points is null'), (lambda: bam(ws=None), 'ws is null'), (lambda: bam(S=None), 'S is null'),
                       (lambda: bam(r=None), 'r is null'), (lambda: bam(stats=None), 'stats'),
                       (lambda: bau(V=1), 'V must be'), (lambda: bau(J=0), 'J must be'), (lambda: bau(sigma=inf), 'sigma_px'), (lambda: bau(lam=nan), 'lambda'),
                       (lambda: bau(kp=None), 'keypoints'), (lambda: bau(cams=None), 'cams'), (lambda: bau(pts=None), 'points is null'),
                       (lambda: bau(dc=None), 'dc is null'), (lambda: bau(out=None), 'points_new')):
        assert call() == -1
        assert word in L.rohm_last_error().decode(), word
    # Q == 0 returns without a launch, whatever the pointers
    assert hyp(Q=0, kp=None, cams=None, pairs=None, samples=None, ws=None, E=None, counts=None, best=None) == 0
    assert mom(Q=0, kp=None, cams=None, pairs=None, E=None, ws=None, out=None) == 0


# ---- 9: the margins of the GPU inputs -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(RR.PAIR_CASES))
def test_margins_of_the_gpu_inputs(name):
    """The conditions the equalities of tests/test_gpu_rig.py rest on: eigen-gap lambda_2 / lambda_9 >= 1e-6, no |d - tau_px| < 1e-6
    px, the two largest |E_i| 1e-9 apart.  At most 5 % of a case's non-degenerate hypotheses may fall outside them."""
    case = RR.build_pair_case(name)
    ref = case['ref']
    live = ref['counts'][..., 0] >= 0
    ok = RR.margins_ok(ref)
    share = 1.0 - ok.sum() / max(1, live.sum())
    print(f'{name}: {int(live.sum())} of {live.size} hypotheses are live, {int(live.sum() - ok.sum())} inside the margins; least gap '
          f'{np.nanmin(ref["gap"]):.2e}, least |d - tau| {ref["margin_tau"].min():.2e} px; best {ref["best"].tolist()[:8]}')
    assert live.any() and (~live).any() and share <= 0.05
    # `best` and the counts are compared for every hypothesis: those rest on the tau margin alone
    assert (ref['margin_tau'][live] >= 1e-6).all()
    assert (case['margin_moments'] >= 1e-6).all()
    for q in range(len(case['pairs'])):                                    # the winner is not a tie between a hypothesis inside and one outside the margins
        if ref['best'][q] >= 0:
            assert ok[q, ref['best'][q]]
