"""CPU: the rule of the SMPL-X fit.  tests/fit_ref.py (the float64 restatement tests/test_gpu_fit.py holds csrc/fit.hip to) against
central finite differences, an independent forward kinematics (`synth._fk_np`) and closed-form cases, and the host logic of
`rohm_amd.fit` (`fit_joints`, `fit_track`, the skeleton file) with the two kernels replaced by the restatement.

Bars.  Jacobian against central differences (step 1e-6): 1e-6 m/rad.  The analytic form is the derivative of the exact
exponential map; the model's Rodrigues takes its angle from |r + 1e-8|, which changes the derivative by at most 1e-8 sqrt(3) /
|theta_k| relative (|theta_k| >= 0.05 here: 3.5e-7) on lever arms below 1 m; the differences themselves are good to
1e-16 / 1e-6 = 1e-10.  E through `synth._fk_np` (true-norm Rodrigues, its own chain): the joints differ by at most
delta = 2e-7 m (the same 1e-8 rad over at most 8 links of at most 1 m, doubled), so |dE| <= 2 sqrt(E_data sum c) delta + sum c
delta^2.  Recovery: 2 mm, the issue's bar."""
import numpy as np
import pytest
import torch

import fit_ref as FR
from rohm_amd.utils import synth

NJ, NX, NROT = FR.NJ, FR.NX, FR.NROT


@pytest.fixture(scope='module')
def tensors():
    return synth.synthetic_smplx_tensors(0)


@pytest.fixture(scope='module')
def mdl(tensors):
    return FR.model(tensors)


def w_prior():
    from rohm_amd.fit import default_w_prior
    return default_w_prior()


def folded_tensors(mdl):
    """A body whose regression is the identity on the handle's own (float32) rest joints and shape directions: `synth._fk_np` of
    it runs on exactly the numbers the restatement has."""
    return {'v_template': torch.from_numpy(mdl['Jt']), 'shapedirs': torch.from_numpy(mdl['Js']), 'J_regressor': torch.eye(NJ, dtype=torch.float64)}


def random_problem(mdl, seed, conf_zero=(), min_theta=0.05):
    g = np.random.Generator(np.random.PCG64(seed))
    theta = g.standard_normal((NJ, 3)) * 0.3
    norm = np.linalg.norm(theta, axis=1, keepdims=True)
    theta = np.where(norm < min_theta, theta / norm * min_theta, theta)
    x = np.concatenate([theta.reshape(-1), g.standard_normal(3)])
    beta = FR._f32(g.standard_normal(10) * 0.5)
    rest = FR.rest_joints(mdl, beta)
    y = FR._f32(FR.fk(mdl, theta, rest)[1] + x[NROT:] + g.standard_normal((NJ, 3)) * 0.02)
    c = g.uniform(0.2, 1.0, size=NJ)
    c[list(conf_zero)] = 0.0
    mean = np.concatenate([np.zeros(3), g.standard_normal(63) * 0.1])
    wsm = np.concatenate([np.zeros(3), np.full(63, 0.05)])
    return x, beta, rest, c, y, mean, wsm


# ---- 1. the Jacobian and the normal equations -------------------------------------------------------------------------------------------
def test_rotation_helpers():
    g = np.random.Generator(np.random.PCG64(0))
    for k in range(200):
        r = FR.random_rotvec(g, np.pi if k % 2 else np.pi * (1 - 1e-7))
        back = FR.log_map(FR.rodrigues(r))
        assert np.abs(FR.rodrigues(back) - FR.rodrigues(r)).max() < 1e-7, (r, back)
    for r in (np.zeros(3), np.array([1e-9, 0, 0]), np.array([0, np.pi, 0]), np.array([np.pi / np.sqrt(2), 0, -np.pi / np.sqrt(2)])):
        assert np.abs(FR.rodrigues(FR.log_map(FR.rodrigues(r))) - FR.rodrigues(r)).max() < 1e-7
    # the right Jacobian: exp(r + d) = exp(r) exp(J_r d) to first order; its series meets the closed form at 1e-6
    # (with the exact exponential, `synth._rodrigues_np`: the model's |r + 1e-8| convention is 1e-8 away from a rotation)
    r, d = np.array([0.3, -0.2, 0.5]), np.array([1e-7, 2e-7, -1e-7])
    lhs = synth._rodrigues_np(r[None])[0].T @ synth._rodrigues_np((r + d)[None])[0]
    want = FR.right_jacobian(r) @ d
    assert np.abs(np.array([lhs[2, 1], lhs[0, 2], lhs[1, 0]]) - want).max() < 1e-12
    a, b = FR.right_jacobian(np.array([0.999999e-6, 0, 0])), FR.right_jacobian(np.array([1.000001e-6, 0, 0]))
    assert np.abs(a - b).max() < 2e-10                    # 1 - cos a rounds to 1e-16 of 1: (1e-16 / a^2) a = 1e-10 in J_r just above 1e-6


@pytest.mark.parametrize('seed', (1, 2, 3))
def test_jacobian_against_central_differences(mdl, seed):
    x, beta, rest, c, y, mean, wsm = random_problem(mdl, seed)
    G, P, _ = FR.residuals(mdl, x, rest, y)
    J = FR.jacobian(mdl, x, G, P)
    num = np.zeros_like(J)
    h = 1e-6
    for i in range(NX):
        e = np.zeros(NX)
        e[i] = h
        num[:, i] = (FR.residuals(mdl, x + e, rest, y)[2] - FR.residuals(mdl, x - e, rest, y)[2]).reshape(-1) / (2 * h)
    err = np.abs(J - num).max()
    print(f'seed {seed}: max |J - central differences| = {err:.3e} (bar 1e-6), max |J| = {np.abs(J).max():.3f}')
    assert err <= 1e-6
    # structure: a joint's rotation moves its strict descendants only; the translation moves every joint alike
    anc = FR.ancestors(mdl['parents'])
    for j in range(NJ):
        for k in range(NJ):
            if k not in anc[j]:
                assert not num[3 * j:3 * j + 3, 3 * k:3 * k + 3].any() or np.abs(num[3 * j:3 * j + 3, 3 * k:3 * k + 3]).max() < 1e-9
    assert all(not anc[j] or 0 in anc[j] for j in range(NJ)) and anc[0] == []


@pytest.mark.parametrize('seed', (4, 5))
def test_normal_equations_are_jtcj_and_half_the_gradient(mdl, seed):
    x, beta, rest, c, y, mean, wsm = random_problem(mdl, seed, conf_zero=(7, 20))
    wp = w_prior()
    H, g, E = FR.normal_equations(mdl, x, rest, c, y, wp, mean, wsm)
    G, P, r = FR.residuals(mdl, x, rest, y)
    J = FR.jacobian(mdl, x, G, P)
    C = np.diag(np.repeat(c, 3))
    D = np.zeros(NX)
    D[:NROT] = np.repeat(wp, 3) + wsm
    assert np.abs(H - (J.T @ C @ J + np.diag(D))).max() <= 1e-12 * np.abs(H).max()
    assert np.array_equal(H, H.T) or np.abs(H - H.T).max() <= 1e-15 * np.abs(H).max()
    # g is half the gradient of E: central differences of E
    h = 1e-6
    num = np.array([(FR.energy(mdl, x + h * e, rest, c, y, wp, mean, wsm) - FR.energy(mdl, x - h * e, rest, c, y, wp, mean, wsm)) / (4 * h)
                    for e in np.eye(NX)])
    print(f'seed {seed}: max |g - dE/2| = {np.abs(g - num).max():.3e} of max |g| = {np.abs(g).max():.3e}')
    assert np.abs(g - num).max() <= 1e-6 * max(np.abs(g).max(), 1.0)


@pytest.mark.parametrize('seed', (6, 7))
def test_energy_through_an_independent_fk(mdl, seed):
    x, beta, rest, c, y, mean, wsm = random_problem(mdl, seed, conf_zero=(3,))
    wp = w_prior()
    theta = x[:NROT].reshape(NJ, 3)
    joints = synth._fk_np(folded_tensors(mdl), synth._rodrigues_np(theta[:1]), theta[1:].reshape(1, 63), beta[None], x[None, NROT:])[0]
    r = joints - y
    data = float((c * (r * r).sum(axis=1)).sum())
    want = data + float((np.repeat(wp, 3) * x[:NROT] ** 2).sum() + (wsm * (x[:NROT] - mean) ** 2).sum())
    got = FR.energy(mdl, x, rest, c, y, wp, mean, wsm)
    delta = 2e-7
    bar = 2.0 * np.sqrt(data * c.sum()) * delta + c.sum() * delta ** 2
    print(f'seed {seed}: E = {got:.6e}, through synth._fk_np {want:.6e}, |difference| {abs(got - want):.3e} (bar {bar:.3e})')
    assert abs(got - want) <= bar


# ---- 2. shape moments -----------------------------------------------------------------------------------------------------------------------
def test_shape_moments_recover_the_true_shape(tensors, mdl):
    from rohm_amd.fit import shape_energy, solve_shape
    N = 6
    g = np.random.Generator(np.random.PCG64(11))
    beta = g.standard_normal(10)
    theta = g.standard_normal((N, NJ, 3)) * 0.4
    transl = g.standard_normal((N, 3))
    params = np.concatenate([theta.reshape(N, -1), transl], axis=1)
    rest = mdl['Jt'] + mdl['Js'] @ beta
    y = np.stack([FR.fk(mdl, theta[i], rest)[1] + transl[i] for i in range(N)])
    conf = g.uniform(0.3, 1.0, size=(N, NJ)).astype(np.float32)
    use = np.array([1, 1, 0, 1, 1, 1], np.uint8)
    keep = FR._f32
    FR._f32 = lambda a: np.asarray(a, dtype=np.float64)                              # targets as float64: no rounding between y and the model
    try:
        rows, tot = FR.shape_moments(mdl, y, conf, params, use)
    finally:
        FR._f32 = keep
    assert not rows[2].any() and rows[[0, 1, 3, 4, 5]].any(axis=1).all() and np.abs(tot - rows.sum(axis=0)).max() == 0.0
    got = solve_shape(tot, 0.0, int(use.sum()))
    print(f'beta from one solve with ridge 0: max |error| = {np.abs(got - beta).max():.3e}')
    assert np.abs(got - beta).max() <= 1e-9
    assert abs(shape_energy(tot, beta, 0.0, 5)) <= 1e-12 * tot[65]
    # the residual term is |y - a - A b|^2 expanded, at any b
    b = g.standard_normal(10)
    want = 0.0
    for i in np.flatnonzero(use):
        a, A = FR.shape_basis(mdl, params[i])
        e = y[i] - a - A @ b
        want += float((conf[i].astype(np.float64) * (e * e).sum(axis=1)).sum())
    assert abs(shape_energy(tot, b, 0.0, 5) - want) <= 1e-10 * want
    # and the linear model is the forward kinematics
    a, A = FR.shape_basis(mdl, params[0])
    assert np.abs(a + A @ beta - y[0]).max() <= 1e-12


# ---- 3. the iteration -------------------------------------------------------------------------------------------------------------------------
RECOVERY = {}


def recovery(tensors, mdl):
    """The issue's recovery check, computed once: 12 frames, body pose ~ N(0, 0.12 rad), any root rotation up to pi, known betas,
    noise-free targets, default weights, 30 iterations."""
    if not RECOVERY:
        joints, theta, transl, betas = FR.make_frames(tensors, 12, seed=21, pose_scale=0.12, beta_scale=0.5)
        traces = {}
        params, report, _ = FR.fit_pose(mdl, joints, None, np.repeat(betas[None], 12, axis=0), w_prior=w_prior(), iters=30, traces=traces)
        RECOVERY.update(joints=joints, theta=theta, transl=transl, betas=betas, params=params, report=report, traces=traces)
    return RECOVERY


def test_energy_never_increases(tensors, mdl):
    rec = recovery(tensors, mdl)
    for i, tr in rec['traces'].items():
        assert len(tr) == 31 and (np.diff(tr) <= 0.0).all(), (i, tr)
        assert tr[0] == rec['report'][i, 1] and tr[-1] == rec['report'][i, 2]
        assert rec['report'][i, 3] == (np.diff(tr) < 0.0).sum()


def test_recovery_within_two_millimetres(tensors, mdl):
    rec = recovery(tensors, mdl)
    assert (rec['report'][:, 0] == 1).all()
    worst = 0.0
    for i in range(12):
        rest = FR.rest_joints(mdl, rec['betas'])
        P = FR.residuals(mdl, rec['params'][i], rest, 0.0)[1] + rec['params'][i, NROT:]
        worst = max(worst, float(np.linalg.norm(P - rec['joints'][i].astype(np.float64), axis=1).max()))
    root_angles = np.linalg.norm(rec['theta'][:, 0], axis=1)
    print(f'recovery: worst joint {worst * 1e3:.3f} mm (bar 2 mm), rms {rec["report"][:, 5].max() * 1e3:.3f} mm; root angles {root_angles.min():.2f} .. '
          f'{root_angles.max():.2f} rad')
    assert root_angles.max() > 2.0
    assert worst <= 2e-3
    assert np.abs(rec['report'][:, 5]).max() <= 2e-3


def test_iters_zero_is_the_start_point(tensors, mdl):
    rec = recovery(tensors, mdl)
    b = np.repeat(rec['betas'][None], 12, axis=0)
    p0, r0, n0 = FR.fit_pose(mdl, rec['joints'], None, b, w_prior=w_prior(), iters=0, want_normal=True)
    assert (r0[:, 1] == r0[:, 2]).all() and not r0[:, 3].any() and (r0[:, 4] == FR.LAMBDA0).all() and n0.shape == (12, NX, NX + 1)
    assert not p0[:, 3:NROT].any() and p0[:, :3].any(axis=1).all()
    # the triad start already has the torso in place: hips and neck within a few centimetres (the body pose is still missing)
    assert r0[:, 5].max() < 0.1
    # an init row is taken as it is, a row that is not finite falls back to the triad
    init = rec['params'].copy()
    init[3] = np.nan
    p1, r1, _ = FR.fit_pose(mdl, rec['joints'], None, b, init=init, w_prior=w_prior(), iters=0)
    assert np.array_equal(p1[[0, 1, 2]], init[[0, 1, 2]]) and np.array_equal(p1[3], p0[3])
    assert np.allclose(r1[[0, 1, 2], 1], rec['report'][[0, 1, 2], 2], rtol=1e-12)


def test_status_rules(tensors, mdl):
    rec = recovery(tensors, mdl)
    N = 6
    joints = rec['joints'][:N].copy()
    conf = np.ones((N, NJ), np.float32)
    conf[0, 5:] = 0.0                                      # 5 joints: fewer than min_joints = 6
    conf[1, 2] = 0.0                                       # a hip is missing: no triad
    joints[2, 12] = np.nan                                 # the neck is not a number: the same
    conf[3, 15] = np.nan                                   # a confidence that is not a number: that joint is unobserved, the frame is fitted
    conf[3, 16] = -1.0
    joints[4] = np.nan                                     # a whole frame of NaN
    joints[5, 1] = joints[5, 2]                            # both hips on one spot: a degenerate triad
    b = np.repeat(rec['betas'][None], N, axis=0)
    p, r, n = FR.fit_pose(mdl, joints, conf, b, w_prior=w_prior(), iters=3, want_normal=True)
    assert r[:, 0].tolist() == [0, 2, 2, 1, 0, 2]
    bad = [0, 1, 2, 4, 5]
    assert not p[bad].any() and not n[bad].any() and np.isnan(r[bad][:, [1, 2, 4, 5]]).all() and not r[bad, 3].any()
    assert np.isfinite(p[3]).all() and np.isfinite(r[3]).all() and r[3, 2] < r[3, 1]
    c, y = FR.observation(joints[3], conf[3])
    assert c[15] == 0 and c[16] == 0 and (c > 0).sum() == 20
    # with an init row a frame without a triad is fitted; a frame with too few joints still is not
    init = np.repeat(rec['params'][:1], N, axis=0)
    p, r, _ = FR.fit_pose(mdl, joints, conf, b, init=init, w_prior=w_prior(), iters=3)
    assert r[:, 0].tolist() == [0, 1, 1, 1, 0, 1]
    assert FR.fit_pose(mdl, joints, conf, b, w_prior=w_prior(), iters=0, min_joints=5)[1][0, 0] == 2       # joints 0..4: a triad needs 12


def test_smoothing_term(tensors, mdl):
    rec = recovery(tensors, mdl)
    b = np.repeat(rec['betas'][None], 3, axis=0)
    prev = rec['params'][:3].copy()
    prev[1] = np.nan                                       # the middle frame has no solution
    wp = w_prior()
    p, r, _ = FR.fit_pose(mdl, rec['joints'][:3], None, b, init=rec['params'][:3], prev=prev, w_prior=wp, w_smooth=0.5, iters=0)
    plain = FR.fit_pose(mdl, rec['joints'][:3], None, b, init=rec['params'][:3], w_prior=wp, iters=0)[1]
    # frames 0 and 2 have only the invalid middle frame as a neighbour: no smoothing term at all
    assert np.array_equal(r[[0, 2]], plain[[0, 2]])
    # frame 1: the mean of frames 0 and 2, body pose only
    m = 0.5 * (prev[0] + prev[2])[3:NROT]
    want = plain[1, 1] + 0.5 * ((rec['params'][1, 3:NROT] - m) ** 2).sum()
    assert abs(r[1, 1] - want) <= 1e-12 * want
    prev[0] = rec['params'][0]
    prev[1] = rec['params'][1]
    prev[2, 5] = np.inf
    r2 = FR.fit_pose(mdl, rec['joints'][:3], None, b, init=rec['params'][:3], prev=prev, w_prior=wp, w_smooth=0.5, iters=0)[1]
    want = plain[1, 1] + 0.5 * ((rec['params'][1, 3:NROT] - prev[0, 3:NROT]) ** 2).sum()
    assert abs(r2[1, 1] - want) <= 1e-12 * want and r2[2, 1] > plain[2, 1] and r2[0, 1] > plain[0, 1]


# ---- 4. fit_joints / fit_track on the restatement ----------------------------------------------------------------------------------------------
@pytest.fixture()
def on_reference(monkeypatch, mdl):
    from rohm_amd import fit
    monkeypatch.setattr(fit, '_native', lambda body_model, device: mdl)
    monkeypatch.setattr(fit, 'fit_pose', FR.torch_fit_pose)
    monkeypatch.setattr(fit, 'shape_moments', FR.torch_shape_moments)
    return fit


def body25(joints, conf=None):
    """BODY_25 arrays whose `OPENPOSE_TO_SMPL` image is `joints` at every SMPL joint but `BODY25_PROXY`, the ones the map fills with
    a neighbour's BODY_25 joint."""
    from rohm_amd.data_loaders.dataloader_video import OPENPOSE_TO_SMPL
    from rohm_amd.fit import BODY25_PROXY
    N = len(joints)
    j25, c25 = np.zeros((N, 25, 3), np.float32), np.zeros((N, 25), np.float32)
    for s, o in enumerate(OPENPOSE_TO_SMPL[:NJ]):
        if s in BODY25_PROXY:
            continue
        j25[:, o] = joints[:, s]
        c25[:, o] = 1.0 if conf is None else conf[:, s]
    return j25, c25


def test_fit_track_keys_and_read_track(on_reference, tensors, mdl):
    from rohm_amd.data_loaders.track import TRACK_KEYS, read_track
    fit = on_reference
    joints = FR.make_frames(tensors, 5, seed=31, pose_scale=0.1, walk=True)[0]
    conf = np.ones((5, NJ), np.float32)
    conf[2, 4:] = 0.0                                      # frame 2: 4 joints
    conf[3, 1] = 0.0                                       # frame 3: no triad -> warm start from frame 4 (or 1; the earlier on ties: 1 is two away)
    skel = dict(joints_3d=joints, joint_conf=conf, fps=30.0, cam2world=np.eye(4), recording_name=np.array('walk'), up_axis=np.array('y'))
    track, res = fit.fit_track(skel, device='cpu', return_result=True, iters=4, smooth_passes=1)
    assert set(track) <= set(TRACK_KEYS)
    assert set(track) == {'global_orient', 'transl', 'body_pose', 'betas', 'valid', 'fps', 'cam2world', 'recording_name', 'up_axis'}
    assert track['valid'].tolist() == [True, True, False, True, True] and res.warm_started.tolist() == [False, False, False, True, False]
    assert track['global_orient'].dtype == np.float32 and track['body_pose'].shape == (5, 63) and track['betas'].shape == (10,)
    assert not track['body_pose'][2].any() and not track['transl'][2].any()
    assert res.report[:, 0].tolist() == [1, 1, 0, 1, 1] and res.energy_history is None
    rec = read_track(track)
    assert rec['valid'].tolist() == track['valid'].tolist() and rec['up_axis'] == 'y' and rec['recording_name'] == 'walk'
    assert res.summary()['fitted'] == 4 and res.summary()['skipped'] == 1 and res.summary()['warm_started'] == 1
    # without cam2world the result is what floor.calibrate_track takes: read_track misses cam2world and nothing else
    del skel['cam2world']
    track = fit.fit_track(skel, device='cpu', iters=1, smooth_passes=0)
    with pytest.raises(ValueError, match=r"missing \['cam2world'\]"):
        read_track(track)
    read_track(dict(track, cam2world=np.eye(4)))
    # times instead of fps
    skel2 = dict(joints_3d=joints, times=np.array([0.0, 0.1, 0.2, 0.35, 0.5]))
    assert np.array_equal(fit.fit_track(skel2, device='cpu', iters=1, smooth_passes=0)['times'], skel2['times'])


def test_fit_track_refusals(on_reference, tensors):
    fit = on_reference
    joints = FR.make_frames(tensors, 3, seed=32)[0]
    ok = dict(joints_3d=joints, fps=30.0)
    with pytest.raises(ValueError, match=r"unknown keys \['global_orient', 'pose'\]"):
        fit.fit_track(dict(ok, pose=1, global_orient=2), device='cpu')
    with pytest.raises(ValueError, match='exactly one of fps and times'):
        fit.fit_track(dict(ok, times=np.arange(3.0)), device='cpu')
    with pytest.raises(ValueError, match='exactly one of fps and times'):
        fit.fit_track(dict(joints_3d=joints), device='cpu')
    with pytest.raises(ValueError, match='joints_3d must be'):
        fit.fit_track(dict(ok, joints_3d=joints[:, :21]), device='cpu')
    with pytest.raises(ValueError, match='joint_conf must be'):
        fit.fit_track(dict(ok, joint_conf=np.ones((3, 25))), device='cpu')
    with pytest.raises(ValueError, match='strictly increasing'):
        fit.fit_track(dict(joints_3d=joints, times=np.array([0.0, 0.2, 0.1])), device='cpu')
    with pytest.raises(ValueError, match='missing'):
        fit.fit_track(dict(fps=30.0), device='cpu')
    with pytest.raises(ValueError, match='betas must be'):
        fit.fit_track(dict(ok, betas=np.zeros(9)), device='cpu')
    # nothing can be fitted: every frame lacks its neck
    conf = np.ones((3, NJ), np.float32)
    conf[:, 12] = 0.0
    with pytest.raises(ValueError, match='no frame could be fitted'):
        fit.fit_track(dict(ok, joint_conf=conf), device='cpu')


def test_fit_track_body25(on_reference, tensors):
    from rohm_amd.data_loaders.dataloader_video import OPENPOSE_TO_SMPL
    fit = on_reference
    joints = FR.make_frames(tensors, 2, seed=33, pose_scale=0.1)[0]
    j25, c25 = body25(joints)
    got_j, got_c, _, times, extra = fit.read_skeleton(dict(joints_3d=j25, joint_conf=c25, fps=10.0))
    assert got_j.shape == (2, NJ, 3) and np.array_equal(got_j, j25[:, OPENPOSE_TO_SMPL[:NJ]])
    real = [s for s in range(NJ) if s not in fit.BODY25_PROXY]
    assert fit.BODY25_PROXY == (3, 6, 9, 13, 14) and np.array_equal(got_j[:, real], joints[:, real])
    assert not got_c[:, list(fit.BODY25_PROXY)].any() and (got_c[:, real] == 1.0).all()
    assert fit.read_skeleton(dict(joints_3d=j25, fps=10.0))[1] is not None            # without joint_conf the proxies are still switched off
    assert times.tolist() == [0.0, 0.1] and extra == {}
    # the same file in SMPL order gives the same fit
    a = fit.fit_track(dict(joints_3d=j25, joint_conf=c25, fps=10.0), device='cpu', iters=2, smooth_passes=0)
    b = fit.fit_track(dict(joints_3d=got_j, joint_conf=got_c, fps=10.0), device='cpu', iters=2, smooth_passes=0)
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_fit_joints_shape_history(on_reference, tensors, mdl):
    fit = on_reference
    joints, _, _, betas = FR.make_frames(tensors, 4, seed=34, pose_scale=0.1, beta_scale=1.0)
    res = fit.fit_joints(joints, fit_shape=True, shape_rounds=2, iters=6, smooth_passes=0, device='cpu')
    h = res.energy_history
    print('energy history:', h, 'betas error', np.abs(res.betas - betas).max())
    assert len(h) == 3 and all(h[i + 1] <= h[i] * (1 + 1e-12) for i in range(2)) and h[-1] < h[0]
    assert res.betas.any() and np.array_equal(res.betas, res.betas.astype(np.float32).astype(np.float64))
