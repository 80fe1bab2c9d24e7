"""TEST INFRASTRUCTURE ONLY: float64 numpy restatement of csrc/fit.hip (`rohm_fit_pose`, `rohm_fit_shape_moments`), the rule
the kernels are held to in tests/test_gpu_fit.py, itself held to finite differences, an independent forward kinematics and
closed-form cases in tests/test_fit_ref.py.  The rules are stated in include/rohm_hip.h.  Inputs are taken as float32 where the
kernels read float32 and every operation is float64.  The iteration (lambda, the eight tries, the acceptance test) follows the
header to the letter; only the order of the sums differs from the kernel's.

`torch_fit_pose` / `torch_shape_moments` wrap the two with the signatures of `rohm_amd.fit.fit_pose` / `shape_moments` on CPU
tensors, so that a test without a GPU can run `fit_joints` and `fit_track` on them."""
import numpy as np

import helpers

NJ, NX, NROT = 22, 69, 66
LAMBDA0, LAMBDA_MIN, LAMBDA_MAX, TRIES, DIAG_EPS, DEGENERATE = 1e-3, 1e-9, 1e8, 8, 1e-9, 1e-9
record = helpers.parity_recorder('fit_parity.json')


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def model(body_tensors):
    """What the `rohm_smplx_t` handle holds for the 22 body joints: Jt [22,3] and Js [22,3,10], the joint regressor folded into
    the template and the first ten shape directions with float64 sums and rounded to float32 (smplx.hip's fold), and parents."""
    jreg = np.asarray(body_tensors['J_regressor'], dtype=np.float64)[:NJ]
    vt = np.asarray(body_tensors['v_template'], dtype=np.float64)
    sd = np.asarray(body_tensors['shapedirs'], dtype=np.float64)[:, :, :10]
    return {'Jt': _f32(jreg @ vt), 'Js': _f32(np.einsum('jv,vck->jck', jreg, sd)), 'parents': [int(p) for p in np.asarray(body_tensors['parents'])[:NJ]]}


# ---- rotations -------------------------------------------------------------------------------------------------------------
def _skew(x, y, z):
    return np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])


def rodrigues(r):
    """smplx_fk.h's convention: angle = |r + 1e-8|, axis = r / angle, R = I + sin K + (1 - cos) K^2."""
    r = np.asarray(r, dtype=np.float64)
    ang = np.sqrt(((r + 1e-8) ** 2).sum())
    K = _skew(*(r / ang))
    return np.eye(3) + np.sin(ang) * K + (1.0 - np.cos(ang)) * (K @ K)


def right_jacobian(r):
    r = np.asarray(r, dtype=np.float64)
    a2 = float(r @ r)
    a = np.sqrt(a2)
    if a < 1e-6:
        p, q = 0.5 - a2 / 24.0, 1.0 / 6.0 - a2 / 120.0
    else:
        p, q = (1.0 - np.cos(a)) / a2, (a - np.sin(a)) / (a2 * a)
    K = _skew(*r)
    return np.eye(3) - p * K + q * (K @ K)


def log_map(R):
    c = (R[0, 0] + R[1, 1] + R[2, 2] - 1.0) * 0.5
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = 0.5 * np.sqrt((v * v).sum())
    ang = np.arctan2(s, c)
    if s >= 1e-6 and c > -0.99:
        return v * (ang / (2.0 * s))
    if c > 0.0:
        return 0.5 * v
    i = 0
    if R[1, 1] > R[i, i]:
        i = 1
    if R[2, 2] > R[i, i]:
        i = 2
    n = np.zeros(3)
    n[i] = np.sqrt(max((R[i, i] - c) / (1.0 - c), 0.0))
    for j in range(3):
        if j != i:
            n[j] = 0.5 * (R[i, j] + R[j, i]) / ((1.0 - c) * n[i])
    sign = -1.0 if float(v @ n) < 0.0 else 1.0
    return sign * n / np.sqrt((n * n).sum()) * ang


def triad(v1, v2, v12):
    """F = [x^ u^ z^] (columns) or None when a norm is below 1e-9."""
    x = v1 - v2
    nx = np.sqrt((x * x).sum())
    if not nx >= DEGENERATE:
        return None
    x = x / nx
    u = v12 - 0.5 * (v1 + v2)
    u = u - float(u @ x) * x
    nu = np.sqrt((u * u).sum())
    if not nu >= DEGENERATE:
        return None
    u = u / nu
    return np.stack([x, u, np.cross(x, u)], axis=1)


# ---- one frame ---------------------------------------------------------------------------------------------------------------
def rest_joints(mdl, beta):
    return mdl['Jt'] + mdl['Js'] @ _f32(beta)


def fk(mdl, theta, rest):
    """(G [22,3,3] world rotations, P [22,3] posed joints without the translation)."""
    R = [rodrigues(theta[k]) for k in range(NJ)]
    G, P = [R[0]], [rest[0]]
    for j in range(1, NJ):
        p = mdl['parents'][j]
        G.append(G[p] @ R[j])
        P.append(P[p] + G[p] @ (rest[j] - rest[p]))
    return np.stack(G), np.stack(P)


def observation(targets, conf):
    """(c [22], y [22,3]) of one frame: a target or confidence that is not finite, or a confidence <= 0, gives c = 0 and y = 0."""
    y = _f32(targets).reshape(NJ, 3)
    c = np.ones(NJ) if conf is None else _f32(conf).reshape(NJ)
    with np.errstate(invalid='ignore'):
        ok = np.isfinite(y).all(axis=1) & np.isfinite(c) & (c > 0.0)
    return np.where(ok, c, 0.0), np.where(ok[:, None], y, 0.0)


def smoothing(prev, i, N, w_smooth):
    """(mean [66], weight [66]): the mean of prev's rotations over the finite neighbours, body pose only."""
    mean, w = np.zeros(NROT), np.zeros(NROT)
    if prev is None:
        return mean, w
    rows = [prev[g] for g in (i - 1, i + 1) if 0 <= g < N and np.isfinite(prev[g]).all()]
    if rows:
        mean[3:] = (np.sum(rows, axis=0) / len(rows))[3:NROT]
        w[3:] = w_smooth
    return mean, w


def residuals(mdl, x, rest, y):
    G, P = fk(mdl, x[:NROT].reshape(NJ, 3), rest)
    return G, P, P + x[NROT:] - y


def energy_of(x, r, c, w_prior, mean, wsm):
    th = x[:NROT]
    return float((c * (r * r).sum(axis=1)).sum() + (np.repeat(w_prior, 3) * th * th).sum() + (wsm * (th - mean) ** 2).sum())


def energy(mdl, x, rest, c, y, w_prior, mean, wsm):
    return energy_of(x, residuals(mdl, x, rest, y)[2], c, w_prior, mean, wsm)


def ancestors(parents):
    anc = [[] for _ in range(NJ)]
    for j in range(1, NJ):
        anc[j] = anc[parents[j]] + [parents[j]]
    return anc


def jacobian(mdl, x, G, P):
    """[66, 69]: d (p_j + t) / d x."""
    J = np.zeros((NROT, NX))
    M = [G[k] @ right_jacobian(x[3 * k:3 * k + 3]) for k in range(NJ)]
    anc = ancestors(mdl['parents'])
    for j in range(NJ):
        for k in anc[j]:
            J[3 * j:3 * j + 3, 3 * k:3 * k + 3] = -_skew(*(P[j] - P[k])) @ M[k]
        J[3 * j:3 * j + 3, NROT:] = np.eye(3)
    return J


def normal_equations(mdl, x, rest, c, y, w_prior, mean, wsm):
    """(H [69,69], g [69], E)."""
    G, P, r = residuals(mdl, x, rest, y)
    J = jacobian(mdl, x, G, P)
    cw = np.repeat(c, 3)
    H = J.T @ (cw[:, None] * J)
    wp = np.repeat(w_prior, 3)
    H[np.arange(NROT), np.arange(NROT)] += wp + wsm
    g = J.T @ (cw * r.reshape(-1))
    g[:NROT] += wp * x[:NROT] + wsm * (x[:NROT] - mean)
    return H, g, energy_of(x, r, c, w_prior, mean, wsm)


def start_point(mdl, rest, c, y, init_row, min_joints):
    """(status, x or None)."""
    if int((c > 0.0).sum()) < min_joints:
        return 0, None
    if init_row is not None and np.isfinite(init_row).all():
        return 1, np.array(init_row, dtype=np.float64)
    if not (c[1] > 0.0 and c[2] > 0.0 and c[12] > 0.0):
        return 2, None
    Fy, Fr = triad(y[1], y[2], y[12]), triad(rest[1], rest[2], rest[12])
    if Fy is None or Fr is None:
        return 2, None
    x = np.zeros(NX)
    x[:3] = log_map(Fy @ Fr.T)
    _, P, _ = residuals(mdl, x, rest, y)
    x[NROT:] = (c[:, None] * (y - P)).sum(axis=0) / c.sum()
    return 1, x


def fit_frame(mdl, rest, c, y, x, w_prior, mean, wsm, iters, trace=None):
    """-> (x, E0, E, accepted, lambda, H0, g0).  `trace`, a list, receives E after every iteration."""
    H, g, E = normal_equations(mdl, x, rest, c, y, w_prior, mean, wsm)
    H0, g0, E0 = H, g, E
    lam, accepted, fresh = LAMBDA0, 0, True
    for _ in range(iters):
        if not fresh:
            H, g, E = normal_equations(mdl, x, rest, c, y, w_prior, mean, wsm)
            fresh = True
        for _ in range(TRIES):
            A = H + lam * np.diag(np.diag(H) + DIAG_EPS)
            ok = False
            try:
                L = np.linalg.cholesky(A)
                d = np.linalg.solve(L.T, np.linalg.solve(L, -g))
                Et = energy(mdl, x + d, rest, c, y, w_prior, mean, wsm)
                ok = bool(Et < E)
            except np.linalg.LinAlgError:
                pass
            if ok:
                x, E = x + d, Et
                lam = max(lam / 10.0, LAMBDA_MIN)
                accepted += 1
                fresh = False
                break
            lam = min(lam * 10.0, LAMBDA_MAX)
        if trace is not None:
            trace.append(E)
    return x, E0, E, accepted, lam, H0, g0


# ---- rohm_fit_pose -------------------------------------------------------------------------------------------------------------
def fit_pose(mdl, targets, conf, betas, init=None, prev=None, w_prior=None, w_smooth=0.0, iters=20, min_joints=6, want_normal=False,
             traces=None):
    """-> (params [N,69], report [N,6], normal [N,69,70] or None).  `traces`, a dict, receives frame -> [E per iteration]."""
    targets = np.asarray(targets).reshape(-1, NJ, 3)
    N = len(targets)
    betas = np.asarray(betas).reshape(N, 10)
    w_prior = np.asarray(w_prior, dtype=np.float64).reshape(NJ)
    init = None if init is None else np.asarray(init, dtype=np.float64).reshape(N, NX)
    prev = None if prev is None else np.asarray(prev, dtype=np.float64).reshape(N, NX)
    params, report = np.zeros((N, NX)), np.zeros((N, 6))
    normal = np.zeros((N, NX, NX + 1)) if want_normal else None
    for i in range(N):
        c, y = observation(targets[i], None if conf is None else np.asarray(conf).reshape(N, NJ)[i])
        rest = rest_joints(mdl, betas[i])
        status, x = start_point(mdl, rest, c, y, None if init is None else init[i], min_joints)
        if status != 1:
            report[i] = (status, np.nan, np.nan, 0.0, np.nan, np.nan)
            continue
        mean, wsm = smoothing(prev, i, N, w_smooth)
        trace = [] if traces is not None else None
        x, E0, E, accepted, lam, H0, g0 = fit_frame(mdl, rest, c, y, x, w_prior, mean, wsm, iters, trace)
        if traces is not None:
            traces[i] = [E0] + trace
        r = residuals(mdl, x, rest, y)[2]
        params[i] = x
        report[i] = (1.0, E0, E, accepted, lam, np.sqrt((c * (r * r).sum(axis=1)).sum() / c.sum()))
        if want_normal:
            normal[i, :, :NX], normal[i, :, NX] = H0, g0
    return params, report, normal


# ---- rohm_fit_shape_moments ------------------------------------------------------------------------------------------------------
def shape_basis(mdl, x):
    """(a [22,3] with the translation, A [22,3,10]): p_j + t = a_j + A_j beta at the pose x."""
    R = [rodrigues(x[3 * k:3 * k + 3]) for k in range(NJ)]
    G, A, a = [R[0]], [mdl['Js'][0]], [mdl['Jt'][0]]
    for j in range(1, NJ):
        p = mdl['parents'][j]
        G.append(G[p] @ R[j])
        A.append(A[p] + G[p] @ (mdl['Js'][j] - mdl['Js'][p]))
        a.append(a[p] + G[p] @ (mdl['Jt'][j] - mdl['Jt'][p]))
    return np.stack(a) + x[NROT:], np.stack(A)


def shape_moments(mdl, targets, conf, params, use):
    """-> (per_frame [N,66], out [66])."""
    targets = np.asarray(targets).reshape(-1, NJ, 3)
    N = len(targets)
    params = np.asarray(params, dtype=np.float64).reshape(N, NX)
    use = np.asarray(use).reshape(N)
    iu = np.triu_indices(10)
    rows = np.zeros((N, 66))
    for i in range(N):
        if not use[i]:
            continue
        c, y = observation(targets[i], None if conf is None else np.asarray(conf).reshape(N, NJ)[i])
        a, A = shape_basis(mdl, params[i])
        e = y - a
        M = np.einsum('j,jci,jck->ik', c, A, A)
        rows[i, :55] = M[iu]
        rows[i, 55:65] = np.einsum('j,jci,jc->i', c, A, e)
        rows[i, 65] = (c * (e * e).sum(axis=1)).sum()
    return rows, rows.sum(axis=0)


# ---- the two as `rohm_amd.fit.fit_pose` / `shape_moments` on CPU tensors -----------------------------------------------------------
def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def torch_fit_pose(mdl, targets, conf, betas, init=None, prev=None, w_prior=None, w_smooth=0.0, iters=20, min_joints=6, want_normal=False):
    import torch
    p, r, n = fit_pose(mdl, _np(targets), _np(conf), _np(betas), _np(init), _np(prev), _np(w_prior), w_smooth, iters, min_joints, want_normal)
    return torch.from_numpy(p), torch.from_numpy(r), None if n is None else torch.from_numpy(n)


def torch_shape_moments(mdl, targets, conf, params, use):
    import torch
    rows, out = shape_moments(mdl, _np(targets), _np(conf), _np(params), _np(use))
    return torch.from_numpy(rows), torch.from_numpy(out)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def random_rotvec(g, max_angle=np.pi):
    """A rotation vector with a uniform direction and an angle uniform in [0, max_angle]."""
    v = g.standard_normal(3)
    return v / np.linalg.norm(v) * g.uniform(0.0, max_angle)


def make_frames(body_tensors, N, seed, pose_scale=0.12, beta_scale=0.0, noise=0.0, root_angle=np.pi, walk=False, centre=(0.2, -0.1, 3.0)):
    """Frames of the synthetic body: body pose ~ N(0, pose_scale), a random root rotation up to `root_angle`, a translation
    about `centre` (3 m in front of a camera), one shape ~ N(0, beta_scale); joints from `synth._fk_np` (an FK independent of this file) of
    the float32-rounded parameters, plus N(0, noise).  `walk`: the pose, root and translation drift slowly, as a recording's do.
    -> (joints [N,22,3] float32, theta [N,22,3], transl [N,3], betas [10])."""
    from rohm_amd.utils import synth
    g = np.random.Generator(np.random.PCG64(seed))
    betas = _f32(g.standard_normal(10) * beta_scale)
    if walk:
        t = np.arange(N)[:, None] / 30.0
        ph, fr = g.uniform(0, 2 * np.pi, size=(1, 63)), g.uniform(0.2, 0.8, size=(1, 63))
        body = pose_scale * np.sqrt(2.0) * np.sin(2 * np.pi * fr * t + ph)
        r0 = random_rotvec(g, root_angle)
        root = r0[None] + 0.3 * np.sin(2 * np.pi * 0.3 * t + g.uniform(0, 2 * np.pi, size=(1, 3)))
        transl = np.array([centre]) + 0.3 * np.sin(2 * np.pi * 0.2 * t + g.uniform(0, 2 * np.pi, size=(1, 3)))
    else:
        body = g.standard_normal((N, 63)) * pose_scale
        root = np.stack([random_rotvec(g, root_angle) for _ in range(N)])
        transl = np.array([centre]) + g.standard_normal((N, 3)) * 0.3
    body, root, transl = _f32(body), _f32(root), _f32(transl)
    Rg = synth._rodrigues_np(root)
    joints = synth._fk_np(body_tensors, Rg, body, np.repeat(betas[None], N, axis=0), transl)
    joints = joints + g.standard_normal(joints.shape) * noise
    theta = np.concatenate([root[:, None], body.reshape(N, 21, 3)], axis=1)
    return joints.astype(np.float32), theta, transl, betas
