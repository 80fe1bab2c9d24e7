"""TEST INFRASTRUCTURE ONLY: float64 numpy restatement of csrc/fit_views.hip (`rohm_fit_views_pose`), the rule the kernel is held to
in tests/test_gpu_fit_views.py, itself held to finite differences, an explicitly stacked Jacobian, closed forms and recovery of
planted bodies in tests/test_fit_views_ref.py.  The rule is stated in include/rohm_fit_views.h.  Inputs are taken as float32 where
the kernel reads float32 and every operation is float64.  The kinematics, the joint Jacobian and the constants of the iteration
are tests/fit_ref.py's, the undistortion is tests/multiview_ref.py's; only the order of the sums differs from the kernel's.

`torch_fit_views_pose` wraps it with the signature of `rohm_amd.fit_views.fit_views_pose` on CPU tensors.  The makers of rigs and
frames for the tests are at the end."""
import numpy as np

import fit_ref as FR
import helpers
import multiview_ref as MR

NJ, NX, NROT, CAM, MAX_VIEWS, NREPORT = FR.NJ, FR.NX, FR.NROT, MR.CAM, 16, 8
SINGULAR = 1e-12
record = helpers.parity_recorder('fit_views_parity.json')


# ---- the pieces of the rule ---------------------------------------------------------------------------------------------------
def observations(kp, cams, conf_min):
    """kp [V,22,3] of one frame (float32 values) -> (a, b, c) [V,22]: normalised coordinates and the confidence, c = 0 (and a = b = 0)
    where unobserved."""
    kp = np.asarray(kp, dtype=np.float32).astype(np.float64)
    with np.errstate(all='ignore'):
        S = MR.observed(kp, conf_min)
        a, b = MR.undistort(cams, kp[..., 0], kp[..., 1])
    return np.where(S, a, 0.0), np.where(S, b, 0.0), np.where(S, kp[..., 2], 0.0)


def smoothing(prev, i, N, w_smooth, w_smooth_t):
    """(mean [69], weight [69]): the mean of prev's rows over the finite neighbours; body pose and translation, not the root."""
    mean, w = np.zeros(NX), np.zeros(NX)
    if prev is None:
        return mean, w
    rows = [prev[g] for g in (i - 1, i + 1) if 0 <= g < N and np.isfinite(prev[g]).all()]
    if rows:
        mean[3:] = (np.sum(rows, axis=0) / len(rows))[3:]
        w[3:NROT] = w_smooth
        w[NROT:] = w_smooth_t
    return mean, w


def rho_of(e2, sigma_px):
    """(rho, rho')."""
    if sigma_px == 0.0:
        return e2, np.ones_like(e2)
    s2 = sigma_px * sigma_px
    q = s2 / (s2 + e2)
    return q * e2, q * q


def project(mdl, x, rest, cams, a, b, c, with_j=False):
    """-> dict: G, P, r [V,22,2], e2 [V,22], zc [V,22], seen [V,22] and behind (an observed joint at z_c <= 0); with_j: A [V,22,2,3]."""
    G, P = FR.fk(mdl, x[:NROT].reshape(NJ, 3), rest)
    X = P + x[NROT:]
    R, t = cams[:, :9].reshape(-1, 3, 3), cams[:, 9:12]
    xc = np.einsum('vik,jk->vji', R, X) + t[:, None]
    seen = c > 0.0
    zc = xc[..., 2]
    with np.errstate(all='ignore'):
        u, w = xc[..., 0] / zc, xc[..., 1] / zc
        fx, fy = cams[:, 12][:, None], cams[:, 13][:, None]
        r = np.stack([fx * (u - a), fy * (w - b)], -1)
        e2 = (r * r).sum(-1)
        out = {'G': G, 'P': P, 'r': r, 'e2': e2, 'zc': zc, 'seen': seen, 'behind': bool((seen & ~(zc > 0.0)).any())}
        if with_j:
            A0 = fx[..., None] * (R[:, None, 0, :] - u[..., None] * R[:, None, 2, :]) / zc[..., None]
            A1 = fy[..., None] * (R[:, None, 1, :] - w[..., None] * R[:, None, 2, :]) / zc[..., None]
            out['A'] = np.stack([A0, A1], -2)
    return out


def energy_of(x, pr, c, w_prior, mean, wsm, sigma_px):
    if pr['behind']:
        return np.inf
    rho, _ = rho_of(pr['e2'], sigma_px)
    th = x[:NROT]
    d = x - mean
    return float(np.where(pr['seen'], c * rho, 0.0).sum() + (np.repeat(w_prior, 3) * th * th).sum() + (wsm * d * d).sum())


def energy(mdl, x, rest, cams, a, b, c, w_prior, mean, wsm, sigma_px):
    return energy_of(x, project(mdl, x, rest, cams, a, b, c), c, w_prior, mean, wsm, sigma_px)


def normal_equations(mdl, x, rest, cams, a, b, c, w_prior, mean, wsm, sigma_px):
    """(H [69,69], g [69], E): per joint W_j = sum_v w A^T A and b_j = sum_v w A^T r, then H = sum_j Jp_j^T W_j Jp_j + diag, g likewise."""
    pr = project(mdl, x, rest, cams, a, b, c, with_j=True)
    E = energy_of(x, pr, c, w_prior, mean, wsm, sigma_px)
    J = FR.jacobian(mdl, x, pr['G'], pr['P'])
    _, drho = rho_of(pr['e2'], sigma_px)
    w = np.where(pr['seen'], c * drho, 0.0)
    A = np.where(pr['seen'][..., None, None], pr['A'], 0.0)
    r = np.where(pr['seen'][..., None], pr['r'], 0.0)
    H, g = np.zeros((NX, NX)), np.zeros(NX)
    for j in range(NJ):
        Wj, bj = np.zeros((3, 3)), np.zeros(3)
        for v in range(len(cams)):
            Wj += w[v, j] * (A[v, j].T @ A[v, j])
            bj += w[v, j] * (A[v, j].T @ r[v, j])
        Jp = J[3 * j:3 * j + 3]
        H += Jp.T @ Wj @ Jp
        g += Jp.T @ bj
    wp = np.concatenate([np.repeat(w_prior, 3), np.zeros(3)])
    H[np.arange(NX), np.arange(NX)] += wp + wsm
    g += wp * x + wsm * (x - mean)
    return H, g, E


def stacked(mdl, x, rest, cams, a, b, c, sigma_px):
    """The data term written out row by row -> (Js [2 V 22, 69], r [2 V 22], w [2 V 22]): H_data = Js^T diag(w) Js, g_data = Js^T (w r)."""
    pr = project(mdl, x, rest, cams, a, b, c, with_j=True)
    J = FR.jacobian(mdl, x, pr['G'], pr['P'])
    _, drho = rho_of(pr['e2'], sigma_px)
    rows, rs, ws = [], [], []
    for v in range(len(cams)):
        for j in range(NJ):
            on = bool(pr['seen'][v, j])
            for h in range(2):
                rows.append(pr['A'][v, j, h] @ J[3 * j:3 * j + 3] if on else np.zeros(NX))
                rs.append(pr['r'][v, j, h] if on else 0.0)
                ws.append(c[v, j] * drho[v, j] if on else 0.0)
    return np.array(rows), np.array(rs), np.array(ws)


def start_translation(mdl, x, rest, cams, a, b, c):
    """The closed-form translation at x's rotations, or None where the 3 x 3 system is singular."""
    _, P = FR.fk(mdl, x[:NROT].reshape(NJ, 3), rest)
    A, rhs = np.zeros(6), np.zeros(3)
    idx = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    for j in range(NJ):
        for v in range(len(cams)):
            if not c[v, j] > 0.0:
                continue
            R, t = cams[v, :9].reshape(3, 3), cams[v, 9:12]
            for h, o in ((0, a[v, j]), (1, b[v, j])):
                n = R[h] - o * R[2]
                d = float(n @ P[j]) + (t[h] - o * t[2])
                A += c[v, j] * np.array([n[i] * n[k] for i, k in idx])
                rhs -= c[v, j] * n * d
    c00, c01, c02 = A[3] * A[5] - A[4] * A[4], A[2] * A[4] - A[1] * A[5], A[1] * A[4] - A[2] * A[3]
    det, tr = A[0] * c00 + A[1] * c01 + A[2] * c02, A[0] + A[3] + A[5]
    if not det > SINGULAR * tr ** 3:
        return None
    return MR.solve3(A, rhs)[0]


def start_point(mdl, rest, cams, a, b, c, init_row, min_obs):
    """(status, x or None), before the check of the start's energy."""
    if int((c > 0.0).sum()) < min_obs:
        return 0, None
    t = init_row[NROT:]
    if not np.isfinite(init_row[:NROT]).all() or not (np.isnan(t).all() or np.isfinite(t).all()):
        return 2, None
    x = np.array(init_row, dtype=np.float64)
    if np.isnan(t).all():
        x[NROT:] = 0.0
        t = start_translation(mdl, x, rest, cams, a, b, c)
        if t is None:
            return 3, None
        x[NROT:] = t
    return 1, x


def fit_frame(mdl, rest, cams, a, b, c, x, w_prior, mean, wsm, sigma_px, iters):
    """fit_ref.fit_frame with this energy -> (x, E0, E, accepted, lambda, H0, g0); E0 infinite: nothing was done."""
    args = (rest, cams, a, b, c, w_prior, mean, wsm, sigma_px)
    H, g, E = normal_equations(mdl, x, *args)
    H0, g0, E0 = H, g, E
    lam, accepted, fresh = FR.LAMBDA0, 0, True
    if not E0 < np.inf:
        return x, E0, E, 0, lam, H0, g0
    for _ in range(iters):
        if not fresh:
            H, g, E = normal_equations(mdl, x, *args)
            fresh = True
        for _ in range(FR.TRIES):
            A = H + lam * np.diag(np.diag(H) + FR.DIAG_EPS)
            ok = False
            try:
                L = np.linalg.cholesky(A)
                d = np.linalg.solve(L.T, np.linalg.solve(L, -g))
                Et = energy(mdl, x + d, *args)
                ok = bool(Et < E)
            except np.linalg.LinAlgError:
                pass
            if ok:
                x, E = x + d, Et
                lam = max(lam / 10.0, FR.LAMBDA_MIN)
                accepted += 1
                fresh = False
                break
            lam = min(lam * 10.0, FR.LAMBDA_MAX)
    return x, E0, E, accepted, lam, H0, g0


# ---- rohm_fit_views_pose ---------------------------------------------------------------------------------------------------------
def fit_views_pose(mdl, keypoints, cams, betas, init, prev=None, w_prior=None, w_smooth=0.0, w_smooth_t=0.0, sigma_px=0.0, conf_min=0.2,
                   iters=20, min_obs=12, want_resid=True, want_normal=False):
    """-> (params [N,69], report [N,8], resid [V,N,22] or None, normal [N,69,70] or None)."""
    kp = np.asarray(keypoints, dtype=np.float32)
    cams = np.asarray(cams, dtype=np.float64)
    V, N = kp.shape[:2]
    assert 1 <= V <= MAX_VIEWS and kp.shape[2:] == (NJ, 3) and cams.shape == (V, CAM)
    betas = np.asarray(betas).reshape(N, 10)
    w_prior = np.asarray(w_prior, dtype=np.float64).reshape(NJ)
    init = np.asarray(init, dtype=np.float64).reshape(N, NX)
    prev = None if prev is None else np.asarray(prev, dtype=np.float64).reshape(N, NX)
    params, report = np.zeros((N, NX)), np.zeros((N, NREPORT))
    resid = np.full((V, N, NJ), np.nan) if want_resid else None
    normal = np.zeros((N, NX, NX + 1)) if want_normal else None
    for i in range(N):
        a, b, c = observations(kp[:, i], cams, conf_min)
        n_obs = float((c > 0.0).sum())
        rest = FR.rest_joints(mdl, betas[i])
        status, x = start_point(mdl, rest, cams, a, b, c, init[i], min_obs)
        if status == 1:
            mean, wsm = smoothing(prev, i, N, w_smooth, w_smooth_t)
            x, E0, E, accepted, lam, H0, g0 = fit_frame(mdl, rest, cams, a, b, c, x, w_prior, mean, wsm, sigma_px, iters)
            if not E0 < np.inf:
                status = 3
        if status != 1:
            report[i] = (status, np.nan, np.nan, 0.0, np.nan, np.nan, n_obs, np.nan)
            continue
        pr = project(mdl, x, rest, cams, a, b, c)
        params[i] = x
        report[i] = (1.0, E0, E, accepted, lam, np.sqrt(np.where(pr['seen'], c * pr['e2'], 0.0).sum() / c.sum()), n_obs, pr['zc'][pr['seen']].min())
        if want_resid:
            resid[:, i] = np.where(pr['seen'], np.sqrt(pr['e2']), np.nan)
        if want_normal:
            normal[i, :, :NX], normal[i, :, NX] = H0, g0
    return params, report, resid, normal


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def torch_fit_views_pose(mdl, keypoints, cams, betas, init, prev=None, w_prior=None, w_smooth=0.0, w_smooth_t=0.0, sigma_px=0.0, conf_min=0.2,
                         iters=20, min_obs=12, want_resid=True, want_normal=False):
    import torch
    out = fit_views_pose(mdl, _np(keypoints), _np(cams), _np(betas), _np(init), _np(prev), _np(w_prior), w_smooth, w_smooth_t, sigma_px, conf_min,
                         iters, min_obs, want_resid, want_normal)
    return tuple(None if o is None else torch.from_numpy(o) for o in out)


def joints_of(mdl, params, betas):
    """The 22 joints [N,22,3] of parameter rows (float64)."""
    out = []
    for x, be in zip(np.asarray(params), np.asarray(betas).reshape(len(params), 10)):
        out.append(FR.fk(mdl, x[:NROT].reshape(NJ, 3), FR.rest_joints(mdl, be))[1] + x[NROT:])
    return np.stack(out)


def fit_views(mdl, keypoints, cams, beta, starts, w_prior, w_smooth, w_smooth_t, sigma_px, conf_min=0.2, iters=30, smooth_passes=1, min_obs=12):
    """`rohm_amd.fit_views.fit_views` without init, restated: with V >= 2 triangulation (multiview_ref) and fit_ref.fit_pose give the
    start; with V == 1, and for frames without one, both rows of `starts` run and the smaller final energy wins; then the smoothing
    passes -> (params, report, resid, back_turned [N] bool)."""
    from rohm_amd.fit import default_w_prior
    kp = np.asarray(keypoints, dtype=np.float32)
    V, N = kp.shape[:2]
    b = np.repeat(np.asarray(beta, dtype=np.float32)[None], N, axis=0)
    kw = dict(w_prior=w_prior, sigma_px=sigma_px, conf_min=conf_min, iters=iters, min_obs=min_obs)
    start = np.full((N, NX), np.nan)
    if V >= 2:
        tri = MR.triangulate(kp, cams, conf_min=conf_min)
        p3, r3, _ = FR.fit_pose(mdl, tri['joints'].astype(np.float32), tri['conf'], b, w_prior=default_w_prior(), iters=iters)
        start[r3[:, 0] == 1] = p3[r3[:, 0] == 1]
    usable = np.isfinite(start).all(axis=1)
    params, report, resid = np.zeros((N, NX)), np.zeros((N, NREPORT)), np.full((V, N, NJ), np.nan)
    back = np.zeros(N, bool)
    if usable.any():
        params, report, resid, _ = fit_views_pose(mdl, kp, cams, b, start, **kw)
    if not usable.all():
        rows = np.flatnonzero(~usable)
        cand = [fit_views_pose(mdl, kp[:, rows], cams, b[rows], np.repeat(starts[q:q + 1], len(rows), axis=0), **kw) for q in (0, 1)]
        ea, eb = (np.where(c[1][:, 0] == 1, c[1][:, 2], np.inf) for c in cand)
        pick = eb < ea
        back[rows] = pick
        for k, i in enumerate(rows):
            params[i], report[i], resid[:, i] = (cand[int(pick[k])][q][k] if q < 2 else cand[int(pick[k])][2][:, k] for q in range(3))
    for _ in range(smooth_passes):
        sol = np.where((report[:, 0] == 1)[:, None], params, np.nan)
        params, report, resid, _ = fit_views_pose(mdl, kp, cams, b, sol, prev=sol, w_smooth=w_smooth, w_smooth_t=w_smooth_t, **kw)
    return params, report, resid, back & (report[:, 0] == 1)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
TARGET = (0.0, 0.0, 1.0)


def make_rig(V, seed, distorted=(), radius=3.5, focal=1000.0):
    """V cameras `radius` metres from the body (multiview_ref.make_rig), the views in `distorted` with lens distortion -> cams [V,24]."""
    from rohm_amd.multiview import pack_cameras
    K, W, D = MR.make_rig(V, seed, True, radius=radius, focal=focal, target=TARGET)
    keep = np.zeros((V, 1))
    keep[list(distorted)] = 1.0
    return pack_cameras(K, W, D * keep)


def facing(cams, view=0, back=False):
    """The root rotation of a body that stands upright in view `view`'s image and faces its camera (or turns its back)."""
    R = cams[view, :9].reshape(3, 3)
    return R.T @ np.diag([-1.0, -1.0, 1.0] if back else [1.0, -1.0, -1.0])


def make_body(body_tensors, N, seed, root_base=None, root_angle=np.pi, pose_scale=0.3, beta_scale=0.0, walk=False, centre=TARGET):
    """Frames of the synthetic body (fit_ref.make_frames' recipe) whose root rotation is `root_base` (default the identity) times a
    random rotation of up to `root_angle` -> (joints [N,22,3] float64 in the world, params [N,69] float64, betas [10])."""
    from rohm_amd.utils import synth
    g = np.random.Generator(np.random.PCG64(seed))
    betas = FR._f32(g.standard_normal(10) * beta_scale)
    base = np.eye(3) if root_base is None else root_base
    if walk:
        t = np.arange(N)[:, None] / 30.0
        ph, fr = g.uniform(0, 2 * np.pi, size=(1, 63)), g.uniform(0.2, 0.8, size=(1, 63))
        body = pose_scale * np.sqrt(2.0) * np.sin(2 * np.pi * fr * t + ph)
        r0 = FR.random_rotvec(g, root_angle)
        wob = r0[None] + 0.2 * np.sin(2 * np.pi * 0.3 * t + g.uniform(0, 2 * np.pi, size=(1, 3)))
        transl = np.array([centre]) + 0.3 * np.sin(2 * np.pi * 0.2 * t + g.uniform(0, 2 * np.pi, size=(1, 3)))
    else:
        body = g.standard_normal((N, 63)) * pose_scale
        wob = np.stack([FR.random_rotvec(g, root_angle) for _ in range(N)])
        transl = np.array([centre]) + g.standard_normal((N, 3)) * 0.2
    root = np.stack([FR.log_map(base @ FR.rodrigues(w)) for w in wob])
    body, root, transl = FR._f32(body), FR._f32(root), FR._f32(transl)
    joints = synth._fk_np(body_tensors, synth._rodrigues_np(root), body, np.repeat(betas[None], N, axis=0), transl)
    return np.asarray(joints, dtype=np.float64), np.concatenate([root, body, transl], axis=1), betas


def make_keypoints(cams, joints, seed, noise_px=2.0, conf=(0.5, 1.0)):
    """World joints [N,22,3] seen by every camera through its distortion, with Gaussian pixel noise and uniform confidences ->
    keypoints [V,N,22,3] float32."""
    g = np.random.Generator(np.random.PCG64(seed))
    N = joints.shape[0]
    px, _ = MR.project(cams, joints.reshape(-1, 3))
    px = px + g.standard_normal(px.shape) * noise_px
    kp = np.concatenate([px, g.uniform(conf[0], conf[1], (len(cams), N * NJ, 1))], -1).astype(np.float32)
    return kp.reshape(len(cams), N, NJ, 3)


def pepper(kp, seed, dead_frame=None):
    """A copy of kp with NaN coordinates, and zero, low, negative and NaN confidences on about one detection in ten; `dead_frame` is
    wholly unobserved."""
    g = np.random.Generator(np.random.PCG64(seed))
    kp = kp.copy()
    flat = kp.reshape(-1, 3)
    M = flat.shape[0]
    k = max(1, M // 40)
    flat[g.choice(M, k, replace=False), 0] = np.nan
    flat[g.choice(M, k, replace=False), 1] = np.inf
    flat[g.choice(M, k, replace=False), 2] = 0.0
    flat[g.choice(M, k, replace=False), 2] = 0.1
    flat[g.choice(M, max(1, k // 2), replace=False), 2] = -0.5
    flat[g.choice(M, max(1, k // 2), replace=False), 2] = np.nan
    if dead_frame is not None:
        kp[:, dead_frame] = np.nan
    return kp


# ---- the cases tests/test_gpu_fit_views.py runs, built once and shared -------------------------------------------------------------------
GPU_CASES = {(1, 1): 20, (2, 3): 20, (3, 70): 10, (16, 2): 20}       # (V, N): iterations


def build_case(body_tensors, V, N):
    """-> dict: kp [V,N,22,3] float32 (2 px of noise, confidences in [0.3, 1], peppered; with N >= 3 frame 1 is unusable), cams (view 0
    distorted), betas [N,10] float32, init [N,69] (the planted rotations off by 0.05 rad, the translation NaN: the kernel solves it),
    truth [N,69], joints [N,22,3]; read-only, cached."""
    key = (V, N)
    if key in _CASES:
        return _CASES[key]
    seed = 500 + 10 * V + N
    cams = make_rig(V, seed, distorted=(0,))
    joints, truth, betas = make_body(body_tensors, N, seed + 1, root_base=facing(cams, 0), root_angle=0.6, beta_scale=0.5)
    kp = pepper(make_keypoints(cams, joints, seed + 2, conf=(0.3, 1.0)), seed + 3, dead_frame=1 if N >= 3 else None)
    g = np.random.Generator(np.random.PCG64(seed + 4))
    init = truth.copy()
    init[:, :NROT] += g.standard_normal((N, NROT)) * 0.05
    init[:, NROT:] = np.nan
    b = np.repeat(betas[None].astype(np.float32), N, axis=0)
    case = {'kp': kp, 'cams': cams, 'betas': b, 'init': init, 'truth': truth, 'joints': joints}
    for arr in case.values():
        arr.setflags(write=False)
    _CASES[key] = case
    return case


_CASES = {}
