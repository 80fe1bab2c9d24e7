"""TEST INFRASTRUCTURE ONLY: float64 numpy restatement of csrc/rig.hip (`rohm_rig_pair_hypotheses`, `rohm_rig_pair_moments`,
`rohm_rig_ba_moments`, `rohm_rig_ba_update`), the rule the kernels are held to in tests/test_gpu_rig.py, itself held to closed
forms, central differences, a stacked dense Jacobian and the recovery of planted rigs in tests/test_rig_ref.py.  The rule is
stated in include/rohm_rig.h.  Inputs are taken as float32 where the kernels read float32 and every operation is float64.  The
eigenvectors come from `numpy.linalg.eigh` (the kernel runs cyclic Jacobi), the sums over points are numpy's.

Besides the kernel's outputs `pair_hypotheses` returns three margins per hypothesis on which the equalities of the GPU tests
rest: `gap` = lambda_2 / lambda_9 (the second-smallest eigenvalue of M over the largest: the eigenvector's conditioning),
`margin_tau` the least |d - tau_px| over the pair's common points, and `margin_sign` the gap between the two largest |E_i| (the
sign rule flips E as a whole when they swap).

`torch_*` wrap the four with the signatures of `rohm_amd.rig`'s kernel wrappers on CPU tensors, so that a test without a GPU can
run `rig.calibrate` on them."""
import numpy as np

import helpers
import multiview_ref as MR

CAM = 24
N_MOM = 47                                             # count, sum d^2, the 45 upper-triangle sums of row^T row
GAP_MIN = 1e-12                                        # a hypothesis whose lambda_2 < GAP_MIN lambda_9 is degenerate
DIAG_EPS = 1e-9
TRI = [(i, j) for i in range(9) for j in range(i, 9)]
record = helpers.parity_recorder('rig_parity.json')


# ---- the pieces ------------------------------------------------------------------------------------------------------------------
def undistorted(keypoints, cams, conf_min=0.2, as_given=False):
    """keypoints [V,N,J,3] -> (a, b) [V,P,2] float64, NaN where rule 1 of rohm_multiview.h does not observe the detection."""
    kp32 = np.asarray(keypoints, dtype=np.float32)
    V = kp32.shape[0]
    kp = (np.asarray(keypoints, dtype=np.float64) if as_given else kp32.astype(np.float64)).reshape(V, -1, 3)
    with np.errstate(all='ignore'):
        S = MR.observed(kp, conf_min)
        a, b = MR.undistort(np.asarray(cams, dtype=np.float64), kp[..., 0], kp[..., 1])
    return np.where(S[..., None], np.stack([a, b], -1), np.nan)


def fix_sign(e):
    """e [...,9]: the sign that makes the largest-magnitude entry positive (the lowest index on ties) -> (e, margin_sign)."""
    mag = np.abs(e)
    k = np.argmax(mag, -1)
    top = np.take_along_axis(e, k[..., None], -1)
    srt = np.sort(mag, -1)
    return np.where(top < 0, -e, e), srt[..., -1] - srt[..., -2]


def smallest_eigenvector(M):
    """M [...,9,9] symmetric -> (e [...,9] with the sign rule, gap lambda_2 / lambda_9, margin_sign)."""
    w, v = np.linalg.eigh(M)
    e, ms = fix_sign(v[..., :, 0])
    with np.errstate(all='ignore'):
        gap = w[..., 1] / w[..., -1]
    return e, gap, ms


def rows_of(x1, x2):
    """x1, x2 [...,2] normalised coordinates -> the epipolar row x2 (x) x1 [...,9] (row-major E: x2^T E x1 = row . E)."""
    h1 = np.concatenate([x1, np.ones(x1.shape[:-1] + (1,))], -1)
    h2 = np.concatenate([x2, np.ones(x2.shape[:-1] + (1,))], -1)
    return (h2[..., :, None] * h1[..., None, :]).reshape(x1.shape[:-1] + (9,))


def sampson(E, x1, x2, scale):
    """E [...,9] against points x1, x2 [P,2] -> d [...,P] in pixels."""
    E = np.asarray(E, dtype=np.float64)[..., None, :]
    a1, b1, a2, b2 = x1[:, 0], x1[:, 1], x2[:, 0], x2[:, 1]
    with np.errstate(all='ignore'):
        l0 = E[..., 0] * a1 + E[..., 1] * b1 + E[..., 2]
        l1 = E[..., 3] * a1 + E[..., 4] * b1 + E[..., 5]
        l2 = E[..., 6] * a1 + E[..., 7] * b1 + E[..., 8]
        m0 = E[..., 0] * a2 + E[..., 3] * b2 + E[..., 6]
        m1 = E[..., 1] * a2 + E[..., 4] * b2 + E[..., 7]
        num = a2 * l0 + b2 * l1 + l2
        return np.abs(num) / np.sqrt(l0 * l0 + l1 * l1 + m0 * m0 + m1 * m1) * scale


def pair_scale(cams, v1, v2):
    return (cams[v1, 12] + cams[v1, 13] + cams[v2, 12] + cams[v2, 13]) / 4.0


# ---- rohm_rig_pair_hypotheses -------------------------------------------------------------------------------------------------------
def pair_hypotheses(keypoints, cams, pairs, samples, conf_min=0.2, tau_px=4.0, as_given=False):
    cams = np.asarray(cams, dtype=np.float64)
    pairs = np.asarray(pairs).reshape(-1, 2)
    samples = np.asarray(samples)
    ab = undistorted(keypoints, cams, conf_min, as_given)
    V, P = ab.shape[:2]
    Q, K = samples.shape[:2]
    E = np.full((Q, K, 9), np.nan)
    counts = np.full((Q, K, 2), -1, np.int64)
    best = np.full(Q, -1, np.int32)
    gap = np.full((Q, K), np.nan)
    margin_tau = np.full((Q, K), np.inf)
    margin_sign = np.full((Q, K), np.inf)
    for q in range(Q):
        v1, v2 = int(pairs[q, 0]), int(pairs[q, 1])
        if not (0 <= v1 < V and 0 <= v2 < V) or v1 == v2:
            continue
        common = np.isfinite(ab[v1]).all(-1) & np.isfinite(ab[v2]).all(-1)
        x1, x2 = ab[v1][common], ab[v2][common]
        s = samples[q].astype(np.int64)
        ok = ((s >= 0) & (s < P)).all(-1)
        sc = np.clip(s, 0, P - 1)
        srt = np.sort(s, -1)
        ok &= (srt[:, 1:] != srt[:, :-1]).all(-1)
        ok &= common[sc].all(-1)
        rows = rows_of(np.where(common[sc][..., None], ab[v1][sc], 0.0), np.where(common[sc][..., None], ab[v2][sc], 0.0))       # [K,8,9]
        M = np.zeros((K, 9, 9))
        for i in range(8):                                                 # in sample order
            M = M + rows[:, i, :, None] * rows[:, i, None, :]
        e, g, ms = smallest_eigenvector(np.where(ok[:, None, None], M, np.eye(9)))
        with np.errstate(invalid='ignore'):
            ok &= g >= GAP_MIN
        d = sampson(e, x1, x2, pair_scale(cams, v1, v2))                   # [K,Pc]
        with np.errstate(invalid='ignore'):
            n = (d <= tau_px).sum(-1)
        E[q] = np.where(ok[:, None], e, np.nan)
        counts[q, :, 0] = np.where(ok, n, -1)
        counts[q, :, 1] = np.where(ok, int(common.sum()), -1)
        gap[q] = np.where(ok, g, np.nan)
        if d.shape[1]:
            with np.errstate(invalid='ignore'):
                margin_tau[q] = np.where(ok, np.nanmin(np.abs(np.where(np.isfinite(d), d, np.inf) - tau_px), -1), np.inf)
        margin_sign[q] = np.where(ok, ms, np.inf)
        if ok.any():
            best[q] = int(np.argmax(counts[q, :, 0]))                      # the first of the largest
    return {'E': E, 'counts': counts, 'best': best, 'gap': gap, 'margin_tau': margin_tau, 'margin_sign': margin_sign}


def margins_ok(res, gap=1e-6, tau=1e-6, sign=1e-9):
    """-> [Q,K] bool: non-degenerate hypotheses on which E and the counts may be compared."""
    live = res['counts'][..., 0] >= 0
    with np.errstate(invalid='ignore'):
        return live & (res['gap'] >= gap) & (res['margin_tau'] >= tau) & (res['margin_sign'] >= sign)


# ---- rohm_rig_pair_moments -----------------------------------------------------------------------------------------------------------
def pair_moments(keypoints, cams, pairs, E, conf_min=0.2, tau_px=4.0, as_given=False, with_margin=False):
    """-> moments [Q,47]: the inliers' count, sum d^2 and the 45 upper-triangle sums of row^T row; a row of NaN for a pair outside
    [0, V) or with v1 = v2."""
    cams = np.asarray(cams, dtype=np.float64)
    pairs = np.asarray(pairs).reshape(-1, 2)
    E = np.asarray(E, dtype=np.float64).reshape(-1, 9)
    ab = undistorted(keypoints, cams, conf_min, as_given)
    V = ab.shape[0]
    out = np.full((len(pairs), N_MOM), np.nan)
    margin = np.full(len(pairs), np.inf)
    for q, (v1, v2) in enumerate(pairs):
        if not (0 <= v1 < V and 0 <= v2 < V) or v1 == v2:
            continue
        common = np.isfinite(ab[v1]).all(-1) & np.isfinite(ab[v2]).all(-1)
        x1, x2 = ab[v1][common], ab[v2][common]
        d = sampson(E[q], x1, x2, pair_scale(cams, v1, v2))
        with np.errstate(invalid='ignore'):
            inl = d <= tau_px
        rows = rows_of(x1[inl], x2[inl])
        out[q, 0] = inl.sum()
        out[q, 1] = (d[inl] ** 2).sum()
        out[q, 2:] = [(rows[:, i] * rows[:, j]).sum() for i, j in TRI]
        if np.isfinite(d).any():
            margin[q] = np.abs(d[np.isfinite(d)] - tau_px).min()
    return (out, margin) if with_margin else out


def refit(moments):
    """One row of `pair_moments` -> E [9] of the inliers (the sign rule applied), or None with fewer than 8 of them."""
    if not np.isfinite(moments).all() or moments[0] < 8:
        return None
    M = np.zeros((9, 9))
    for k, (i, j) in enumerate(TRI):
        M[i, j] = M[j, i] = moments[2 + k]
    return smallest_eigenvector(M)[0]


# ---- bundle adjustment -----------------------------------------------------------------------------------------------------------------
def rodrigues(r):
    """fit_math.h's rodrigues64: angle = |r + 1e-8|, axis = r / angle."""
    r = np.asarray(r, dtype=np.float64)
    ang = np.sqrt(((r + 1e-8) ** 2).sum())
    x, y, z = r / ang
    K = np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])
    return np.eye(3) + np.sin(ang) * K + (1.0 - np.cos(ang)) * (K @ K)


def cross_matrix(y):
    return np.array([[0.0, -y[2], y[1]], [y[2], 0.0, -y[0]], [-y[1], y[0], 0.0]])


def ba_terms(cam, X, a, b):
    """One view at one point -> r [2], J_X [2,3], J_c [2,6], z_c."""
    R, t = cam[:9].reshape(3, 3), cam[9:12]
    Y = R @ X
    xc = Y + t
    u, v = xc[0] / xc[2], xc[1] / xc[2]
    A = np.array([[cam[12] / xc[2], 0.0, -cam[12] * u / xc[2]], [0.0, cam[13] / xc[2], -cam[13] * v / xc[2]]])
    r = np.array([cam[12] * (u - a), cam[13] * (v - b)])
    return r, A @ R, np.concatenate([-A @ cross_matrix(Y), A], 1), xc[2]


def rho(e2, sigma_px):
    """Geman-McClure of rohm_fit_views.h -> (rho, rho')."""
    if sigma_px > 0.0:
        q = sigma_px * sigma_px / (sigma_px * sigma_px + e2)
        return q * e2, q * q
    return e2, np.ones_like(e2)


def ba_problem(keypoints, cams, points, conf_min=0.2, as_given=False):
    """-> ab [V,P,2] (NaN where unobserved), c [V,P], inside [P]: the points of the problem (finite, two observed views or more)."""
    kp32 = np.asarray(keypoints, dtype=np.float32)
    V = kp32.shape[0]
    ab = undistorted(keypoints, cams, conf_min, as_given)
    c = (np.asarray(keypoints, dtype=np.float64) if as_given else kp32.astype(np.float64)).reshape(V, -1, 3)[..., 2]
    X = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    obs = np.isfinite(ab).all(-1)
    inside = np.isfinite(X).all(-1) & (obs.sum(0) >= 2)
    return ab, c, obs & inside[None], inside, X


def ba_energy(keypoints, cams, points, conf_min=0.2, sigma_px=10.0, as_given=False):
    cams = np.asarray(cams, dtype=np.float64)
    ab, c, obs, inside, X = ba_problem(keypoints, cams, points, conf_min, as_given)
    E = 0.0
    for v in range(cams.shape[0]):
        m = obs[v]
        with np.errstate(all='ignore'):
            r, e2 = MR.residual(cams[v], X[m], ab[v, m, 0], ab[v, m, 1])
        E += (c[v, m] * rho(e2, sigma_px)[0]).sum()
    return float(E)


def ba_normal(keypoints, cams, points, conf_min=0.2, sigma_px=10.0, lam=1e-3, as_given=False):
    """The per-point and per-camera blocks: U [V,6,6], gc [V,6], Hpp [P,3,3] (undamped), gp [P,3], W [V,P,6,3] (= H_cp), E, n."""
    cams = np.asarray(cams, dtype=np.float64)
    V = cams.shape[0]
    ab, c, obs, inside, X = ba_problem(keypoints, cams, points, conf_min, as_given)
    P = X.shape[0]
    U, gc = np.zeros((V, 6, 6)), np.zeros((V, 6))
    Hpp, gp, W = np.zeros((P, 3, 3)), np.zeros((P, 3)), np.zeros((V, P, 6, 3))
    E, n = 0.0, 0
    for p in np.flatnonzero(inside):
        for v in np.flatnonzero(obs[:, p]):
            r, JX, Jc, zc = ba_terms(cams[v], X[p], ab[v, p, 0], ab[v, p, 1])
            n += 1
            if not zc > 0.0:                                               # behind the camera: +inf, and nothing else
                E += np.inf
                continue
            rh, drh = rho(np.float64(r @ r), sigma_px)
            E += c[v, p] * rh
            w = c[v, p] * drh
            U[v] += w * Jc.T @ Jc
            gc[v] += w * Jc.T @ r
            Hpp[p] += w * JX.T @ JX
            gp[p] += w * JX.T @ r
            W[v, p] = w * Jc.T @ JX
    return {'U': U, 'gc': gc, 'Hpp': Hpp, 'gp': gp, 'W': W, 'E': float(E), 'n': n, 'inside': inside, 'obs': obs, 'X': X}


def _damped_inverse(Hpp, lam):
    Hd = Hpp + lam * np.einsum('pi,ij->pij', np.einsum('pii->pi', Hpp) + DIAG_EPS, np.eye(3))
    return np.linalg.inv(Hd)


def ba_moments(keypoints, cams, points, conf_min=0.2, sigma_px=10.0, lam=1e-3, as_given=False):
    """-> S [6V,6V], r [6V], E, n_obs: the reduced camera system with the points eliminated."""
    t = ba_normal(keypoints, cams, points, conf_min, sigma_px, lam, as_given)
    V = t['U'].shape[0]
    ins = t['inside']
    S, r = np.zeros((6 * V, 6 * V)), t['gc'].reshape(-1).copy()
    for v in range(V):
        S[6 * v:6 * v + 6, 6 * v:6 * v + 6] = t['U'][v] + lam * np.diag(np.diag(t['U'][v]) + DIAG_EPS)
    if ins.any():
        Hinv = _damped_inverse(t['Hpp'][ins], lam)
        Wc = t['W'][:, ins].transpose(1, 0, 2, 3).reshape(-1, 6 * V, 3)      # [p, 6V, 3]
        Z = Wc @ Hinv
        S -= np.einsum('pia,pja->ij', Z, Wc)
        r -= np.einsum('pia,pa->i', Z, t['gp'][ins])
    return {'S': S, 'r': r, 'E': t['E'], 'n_obs': t['n']}


def ba_update(keypoints, cams, points, dc, conf_min=0.2, sigma_px=10.0, lam=1e-3, as_given=False):
    """-> points_new [P,3] (a point outside the problem passes through as given), cams_new [V,24]."""
    cams = np.asarray(cams, dtype=np.float64)
    dc = np.asarray(dc, dtype=np.float64).reshape(-1, 6)
    t = ba_normal(keypoints, cams, points, conf_min, sigma_px, lam, as_given)
    ins = t['inside']
    out = t['X'].copy()
    if ins.any():
        Hinv = _damped_inverse(t['Hpp'][ins], lam)
        rhs = t['gp'][ins] + np.einsum('vpia,vi->pa', t['W'][:, ins], dc)
        out[ins] = t['X'][ins] - np.einsum('pab,pb->pa', Hinv, rhs)
    new = cams.copy()
    for v in range(cams.shape[0]):
        new[v, :9] = (rodrigues(dc[v, :3]) @ cams[v, :9].reshape(3, 3)).reshape(9)
        new[v, 9:12] = cams[v, 9:12] + dc[v, 3:]
    return out, new


# ---- the four as `rohm_amd.rig`'s kernel wrappers on CPU tensors ------------------------------------------------------------------------
def torch_pair_hypotheses(keypoints, cams, pairs, samples, conf_min=0.2, tau_px=4.0):
    import torch
    r = pair_hypotheses(keypoints.numpy(), cams.numpy(), pairs.numpy(), samples.numpy(), conf_min, tau_px)
    return torch.from_numpy(r['E']), torch.from_numpy(r['counts']), torch.from_numpy(r['best'])


def torch_pair_moments(keypoints, cams, pairs, E, conf_min=0.2, tau_px=4.0):
    import torch
    return torch.from_numpy(pair_moments(keypoints.numpy(), cams.numpy(), pairs.numpy(), E.numpy(), conf_min, tau_px))


def torch_ba_moments(keypoints, cams, points, conf_min=0.2, sigma_px=10.0, lam=1e-3):
    import torch
    r = ba_moments(keypoints.numpy(), cams.numpy(), points.numpy(), conf_min, sigma_px, lam)
    return torch.from_numpy(r['S']), torch.from_numpy(r['r']), torch.tensor([r['E'], float(r['n_obs'])], dtype=torch.float64)


def torch_ba_update(keypoints, cams, points, dc, conf_min=0.2, sigma_px=10.0, lam=1e-3):
    import torch
    X, c = ba_update(keypoints.numpy(), cams.numpy(), points.numpy(), dc.numpy(), conf_min, sigma_px, lam)
    return torch.from_numpy(X.reshape(tuple(points.shape))), torch.from_numpy(c)


def on_reference(monkeypatch):
    """Put the restatement under `rohm_amd.rig` and `rohm_amd.multiview`: the host logic then runs without a GPU."""
    from rohm_amd import multiview, rig
    monkeypatch.setattr(multiview, 'triangulate', MR.torch_triangulate)
    monkeypatch.setattr(multiview, 'view_residuals', MR.torch_view_residuals)
    monkeypatch.setattr(rig, 'pair_hypotheses', torch_pair_hypotheses)
    monkeypatch.setattr(rig, 'pair_moments', torch_pair_moments)
    monkeypatch.setattr(rig, 'ba_moments', torch_ba_moments)
    monkeypatch.setattr(rig, 'ba_update', torch_ba_update)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def walking_body(N, J, seed, radius=1.2, centre=(0.0, 0.0, 1.0)):
    """A J-point "body" (a fixed cloud some 0.5 x 0.3 x 1.7 m) that walks a circle of `radius` and turns with it -> X [N,J,3]."""
    g = np.random.Generator(np.random.PCG64(seed))
    body = g.uniform(-1.0, 1.0, (J, 3)) * np.array([0.25, 0.15, 0.85])
    sway = g.standard_normal((N, J, 3)) * 0.03                             # limbs move
    phi = np.linspace(0.0, 2.0 * np.pi, N, endpoint=False) + g.uniform(0, 2 * np.pi)
    c, s = np.cos(phi), np.sin(phi)
    Rz = np.stack([np.stack([-s, -c, 0 * c], -1), np.stack([c, -s, 0 * c], -1), np.stack([0 * c, 0 * c, 1 + 0 * c], -1)], -2)   # [N,3,3]
    X = np.einsum('nij,nkj->nki', Rz, body[None] + sway)
    return X + np.array(centre) + radius * np.stack([c, s, 0 * c], -1)[:, None]


def make_scene(V, N, J, seed, noise_px=2.0, outlier_share=0.0, distortion=True):
    """-> (camera_mtx, world2cam, dist, keypoints [V,N,J,3] float32, X [N,J,3]): `MR.make_rig` cameras that see a walking body with
    Gaussian pixel noise; `outlier_share` of each view's detections are moved by 60..300 px."""
    K, W, D = MR.make_rig(V, seed, distortion)
    from rohm_amd.multiview import pack_cameras
    cams = pack_cameras(K, W, D)
    X = walking_body(N, J, seed + 1)
    g = np.random.Generator(np.random.PCG64(seed + 2))
    px, depth = MR.project(cams, X.reshape(-1, 3))
    assert (depth > 0.5).all()
    px = px + g.standard_normal(px.shape) * noise_px
    bad = g.uniform(size=px.shape[:2]) < outlier_share
    ang, rad = g.uniform(0, 2 * np.pi, px.shape[:2]), g.uniform(60.0, 300.0, px.shape[:2])
    px = px + np.where(bad[..., None], np.stack([rad * np.cos(ang), rad * np.sin(ang)], -1), 0.0)
    kp = np.concatenate([px, g.uniform(0.5, 1.0, px.shape[:2] + (1,))], -1).astype(np.float32)
    return K, W, D, kp.reshape(V, N, J, 3), X


def rig_errors(world2cam, W_true, ref, neighbour):
    """An estimated rig in the reference camera's frame against the planted one -> (worst rotation error in degrees, worst camera
    centre error in metres after fixing the scale from the true ref-neighbour baseline)."""
    rel = W_true @ np.linalg.inv(W_true[ref])[None]                        # the planted rig with the reference camera as the world
    C_true = -np.einsum('vji,vj->vi', rel[:, :3, :3], rel[:, :3, 3])
    C = -np.einsum('vji,vj->vi', world2cam[:, :3, :3], world2cam[:, :3, 3])
    C = C * (np.linalg.norm(C_true[neighbour]) / np.linalg.norm(C[neighbour]))
    rot = 0.0
    for v in range(len(rel)):
        dR = world2cam[v, :3, :3] @ rel[v, :3, :3].T
        rot = max(rot, np.degrees(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0))))
    return rot, float(np.linalg.norm(C - C_true, axis=-1).max())


# ---- the recovery cases of tests/test_rig_ref.py and their bars (its docstring says where they come from) -------------------------------
# name: (V, N, noise px, outlier share, seed); bars: (worst rotation in degrees, worst camera centre in metres)
RECOVERY = {'plain': (4, 60, 2.0, 0.0, 500), 'outliers_10': (4, 60, 2.0, 0.1, 501), 'six_views_outliers_20': (6, 30, 2.0, 0.2, 502),
            'three_views': (3, 20, 1.0, 0.05, 503)}
RECOVERY_BARS = {'plain': (0.06, 0.007), 'outliers_10': (0.13, 0.008), 'six_views_outliers_20': (0.15, 0.008), 'three_views': (0.08, 0.006)}


# ---- the cases tests/test_gpu_rig.py runs, built once and shared ------------------------------------------------------------------------
# pair kernels: name: (V, N, J, Q, K, seed).  Q = 1, 3, 120 and 6 are all the pairs of V views.  The seeds are chosen on the CPU
# (tests/test_rig_ref.py::test_margins_of_the_gpu_inputs) so that at most 5 % of a case's non-degenerate hypotheses fall inside the
# margins; a seed that stops holding is replaced here with a comment, never skipped at run time.
PAIR_CASES = {
    'one_pair': (2, 1, 22, 1, 3, 301),
    'three_views': (3, 5, 22, 3, 40, 302),
    'sixteen_views': (16, 2, 22, 120, 5, 303),
    'many_points': (4, 70, 25, 6, 33, 304),
}
# bundle adjustment: name: (V, P as (N, J), seed).  (4, 1750) spans 110 workgroups, the last ragged; (3, 4400) gives a workgroup
# more than one tile of points.
BA_CASES = {
    'two_views': (2, 1, 22, 311),
    'three_views': (3, 5, 22, 312),
    'sixteen_views': (16, 2, 22, 313),
    'many_points': (4, 70, 25, 314),
    'many_tiles': (3, 200, 22, 315),
}
_CASES = {}


def draw_samples(ab, pairs, K, seed, min_gap=0.0, tries=40):
    """[Q,K,8] int32 indices drawn without repeats from each pair's common points (zeros where there are fewer than 8 of them).
    `min_gap`: a sample whose eigen-gap lambda_2 / lambda_9 is below it is drawn again, up to `tries` times -- one random eight-point
    sample in ten has a gap below 1e-6 whatever the scene, which is a property of the inputs, settled here on the CPU as a seed is."""
    g = np.random.Generator(np.random.PCG64(seed))
    out = np.zeros((len(pairs), K, 8), np.int32)
    for q, (v1, v2) in enumerate(pairs):
        idx = np.flatnonzero(np.isfinite(ab[v1]).all(-1) & np.isfinite(ab[v2]).all(-1))
        if len(idx) < 8:
            continue
        for k in range(K):
            for _ in range(tries):
                s = g.choice(idx, 8, replace=False)
                rows = rows_of(ab[v1][s], ab[v2][s])
                w = np.linalg.eigvalsh(rows.T @ rows)
                if w[1] >= min_gap * w[-1]:
                    break
            out[q, k] = s
    return out


def build_pair_case(name):
    """-> {'keypoints', 'cams' (identity extrinsics: the pair kernels read the intrinsics only), 'pairs', 'samples', 'ref'
    (`pair_hypotheses`), 'E_best' [Q,9] (NaN -> the first live hypothesis' E, else zeros), 'ref_moments', 'margin_moments'}; cached."""
    if name in _CASES:
        return _CASES[name]
    from rohm_amd.multiview import pack_cameras
    V, N, J, Q, K, seed = PAIR_CASES[name]
    Kc, W, D = MR.make_rig(V, seed, True, radius=3.0)                      # a wide cloud seen from near: well-conditioned samples exist
    true = pack_cameras(Kc, W, D)
    kp, _ = MR.make_views(true, N, J, seed + 1000, noise_px=2.0, spread=1.5)
    kp = MR.salt(MR.plant_outliers(kp, 1 if V > 2 else 0, seed + 2000)[0], seed + 3000) if N * J > 22 else MR.salt(kp, seed + 3000)
    if N >= 3:                                                             # salt() blinds frame 1; give it back to all but view 0
        kp[1:, 1, :, 2] = 0.9
    cams = pack_cameras(Kc, np.broadcast_to(np.eye(4), (V, 4, 4)), D)
    pairs = np.stack(np.triu_indices(V, 1), 1).astype(np.int32)
    assert len(pairs) == Q
    ab = undistorted(kp, cams)
    samples = draw_samples(ab, pairs, K, seed + 4000, min_gap=4e-6)
    P = N * J
    # planted degenerate samples, one clause each, in the last pair's first hypotheses (and a pair of their own where Q allows)
    s = samples[-1]
    both = np.isfinite(ab[pairs[-1, 0]]).all(-1) & np.isfinite(ab[pairs[-1, 1]]).all(-1)
    hidden = np.flatnonzero(~both)
    if K >= 5:
        s[0, 3] = P                                                        # outside [0, N J)
        s[1, 0] = -1
        s[2, 5] = s[2, 1]                                                  # repeated
        if len(hidden):
            s[3, 7] = hidden[0]                                            # not common to both views
        s[4] = s[4, 0]                                                     # rank 1: lambda_2 = 0 (and repeated)
    elif len(hidden):
        s[0, 7] = hidden[0]
    if Q >= 3:
        pairs = pairs.copy()
        pairs[1] = (pairs[1, 0], V)                                        # outside [0, V)
    if Q >= 6:
        pairs[2] = (2, 2)                                                  # v1 = v2
    ref = pair_hypotheses(kp, cams, pairs, samples)
    E_best = np.zeros((Q, 9))
    for q in range(Q):
        live = np.flatnonzero(ref['counts'][q, :, 0] >= 0)
        if ref['best'][q] >= 0:
            E_best[q] = ref['E'][q, ref['best'][q]]
        elif len(live):
            E_best[q] = ref['E'][q, live[0]]
    if Q >= 6:
        E_best[3] = np.nan                                                 # an E that is not finite: no inliers
    mom, mm = pair_moments(kp, cams, pairs, E_best, with_margin=True)
    case = {'keypoints': kp, 'cams': cams, 'pairs': pairs, 'samples': samples, 'ref': ref, 'E_best': E_best, 'ref_moments': mom,
            'margin_moments': mm}
    for a in (kp, cams, pairs, samples, E_best):
        a.setflags(write=False)
    _CASES[name] = case
    return case


def build_ba_case(name):
    """-> {'keypoints', 'cams' (the planted rig, disturbed), 'points' (the planted points, disturbed, some NaN), 'dc' [V,6]}; cached.
    Salted keypoints, so some entries are unobserved and some points have fewer than two views."""
    key = 'ba_' + name
    if key in _CASES:
        return _CASES[key]
    from rohm_amd.multiview import pack_cameras
    V, N, J, seed = BA_CASES[name]
    g = np.random.Generator(np.random.PCG64(seed + 5))
    Kc, W, D = MR.make_rig(V, seed, True)
    true = pack_cameras(Kc, W, D)
    kp, X = MR.make_views(true, N, J, seed + 1000, noise_px=2.0)
    kp = MR.salt(MR.plant_outliers(kp, 1, seed + 2000)[0] if V > 2 else kp, seed + 3000)
    cams = true.copy()
    for v in range(V):                                                     # half a degree and a centimetre off
        cams[v, :9] = (rodrigues(g.standard_normal(3) * 0.01) @ true[v, :9].reshape(3, 3)).reshape(9)
        cams[v, 9:12] += g.standard_normal(3) * 0.01
    points = (X + g.standard_normal(X.shape) * 0.01).reshape(-1, 3)
    points[g.choice(len(points), max(1, len(points) // 10), replace=False)] = np.nan
    points[0, 1] = np.inf
    dc = g.standard_normal((V, 6)) * 1e-3
    case = {'keypoints': kp, 'cams': cams, 'points': points, 'dc': dc}
    for a in (kp, cams, points, dc):
        a.setflags(write=False)
    _CASES[key] = case
    return case
