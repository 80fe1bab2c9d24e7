"""TEST INFRASTRUCTURE ONLY: float64 numpy restatement of csrc/multiview.hip (`rohm_mv_triangulate`, `rohm_mv_residuals`), the
rule the kernels are held to in tests/test_gpu_multiview.py, itself held to closed forms, finite differences and recovery of
planted points in tests/test_multiview_ref.py.  The rule is stated in include/rohm_multiview.h.  Inputs are taken as float32
where the kernels read float32 and every operation is float64; it is vectorised over the points and the pairs (1 750 points x
120 pairs take well under a second).  Only the order of the sums over the views of the refinement differs from the kernel's.

Besides the kernel's outputs `triangulate` returns three margins per point, on which the equality of the discrete outputs
rests: `margin_tau` the least |e_v - tau_px| over all scored (pair, view) entries, `margin_angle` the least
| |d1 x d2| - sin(min_angle) | over the pairs of observed views, `margin_cost` the relative cost gap between the winner and the
best other candidate with the same count (infinite where there is none).

`torch_triangulate` / `torch_view_residuals` wrap the two with the signatures of `rohm_amd.multiview.triangulate` /
`view_residuals` on CPU tensors, so that a test without a GPU can run `triangulate_views` on them."""
import numpy as np

import helpers

MAX_VIEWS, MAX_PAIRS, CAM = 16, 120, 24
record = helpers.parity_recorder('multiview_parity.json')


# ---- the pieces of the rule ---------------------------------------------------------------------------------------------------
def pairs_of(V):
    """The pairs v1 < v2 in lexicographic order -> (v1 [Q], v2 [Q])."""
    v1, v2 = np.triu_indices(V, 1)
    return v1, v2


def observed(kp, conf_min):
    x, y, c = kp[..., 0], kp[..., 1], kp[..., 2]
    with np.errstate(invalid='ignore'):
        return np.isfinite(x) & np.isfinite(y) & np.isfinite(c) & (c > conf_min)


def _col(cams, k, like):
    return cams[:, k].reshape((-1,) + (1,) * (like.ndim - 1))


def undistort(cams, px, py):
    """Pixels [V,...] -> normalised (a, b): five fixed-point iterations of the inverse of the k1 k2 p1 p2 k3 model."""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = (_col(cams, k, px) for k in range(12, 21))
    x0, y0 = (px - cx) / fx, (py - cy) / fy
    x, y = x0, y0
    for _ in range(5):
        r2 = x * x + y * y
        icd = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
        x, y = (x0 - dx) * icd, (y0 - dy) * icd
    return x, y


def distort(cams, a, b):
    """Normalised (a, b) [V,...] -> pixels with the forward model."""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = (_col(cams, k, a) for k in range(12, 21))
    r2 = a * a + b * b
    g = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
    ud = a * g + 2.0 * p1 * a * b + p2 * (r2 + 2.0 * a * a)
    vd = b * g + p1 * (r2 + 2.0 * b * b) + 2.0 * p2 * a * b
    return fx * ud + cx, fy * vd + cy


def rays(cams, a, b):
    """-> origins o [V,3], unit directions d [V,P,3]."""
    R, t = cams[:, :9].reshape(-1, 3, 3), cams[:, 9:12]
    o = -np.einsum('vji,vj->vi', R, t)
    d = R[:, None, 0, :] * a[..., None] + R[:, None, 1, :] * b[..., None] + R[:, None, 2, :]
    return o, d / np.sqrt((d * d).sum(-1))[..., None]


def solve3(A, b):
    """x = A^-1 b through the cofactors of the symmetric A [...,6] = (a00, a01, a02, a11, a12, a22) -> (x [...,3], trace(A^-1))."""
    a00, a01, a02, a11, a12, a22 = (A[..., k] for k in range(6))
    c00 = a11 * a22 - a12 * a12
    c01 = a02 * a12 - a01 * a22
    c02 = a01 * a12 - a02 * a11
    c11 = a00 * a22 - a02 * a02
    c12 = a01 * a02 - a00 * a12
    c22 = a00 * a11 - a01 * a01
    det = a00 * c00 + a01 * c01 + a02 * c02
    x = np.stack([(c00 * b[..., 0] + c01 * b[..., 1] + c02 * b[..., 2]) / det,
                  (c01 * b[..., 0] + c11 * b[..., 1] + c12 * b[..., 2]) / det,
                  (c02 * b[..., 0] + c12 * b[..., 1] + c22 * b[..., 2]) / det], -1)
    return x, (c00 + c11 + c22) / det


def ray_terms(w, o, d):
    """w (I - d d^T) [...,6] and w (I - d d^T) o [...,3]."""
    od = (d * o).sum(-1)
    A = np.stack([w * (1.0 - d[..., 0] * d[..., 0]), w * (-d[..., 0] * d[..., 1]), w * (-d[..., 0] * d[..., 2]),
                  w * (1.0 - d[..., 1] * d[..., 1]), w * (-d[..., 1] * d[..., 2]), w * (1.0 - d[..., 2] * d[..., 2])], -1)
    return A, w[..., None] * (o - d * od[..., None])


def residual(cam, X, a, b, with_j=False):
    """One view (cam [24]) at X [...,3]: r [...,2], |r|^2 (infinite when z_c <= 0) and, on request, the Jacobian [...,2,3]."""
    R, t = cam[:9].reshape(3, 3), cam[9:12]
    xc, yc, zc = (X @ R[k] + t[k] for k in range(3))
    u, v = xc / zc, yc / zc
    r = np.stack([cam[12] * (u - a), cam[13] * (v - b)], -1)
    e2 = np.where(zc > 0.0, r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1], np.inf)
    if not with_j:
        return r, e2
    J = np.stack([cam[12] * (R[0] - u[..., None] * R[2]) / zc[..., None], cam[13] * (R[1] - v[..., None] * R[2]) / zc[..., None]], -2)
    return r, e2, J


def _normal(J, w):
    """sum-ready terms of one view: w J^T J as (00, 01, 02, 11, 12, 22) [...,6]."""
    j0, j1 = J[..., 0, :], J[..., 1, :]
    idx = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    return np.stack([w * (j0[..., i] * j0[..., k] + j1[..., i] * j1[..., k]) for i, k in idx], -1)


# ---- rohm_mv_triangulate ---------------------------------------------------------------------------------------------------------
def triangulate(keypoints, cams, conf_min=0.2, tau_px=10.0, min_angle_rad=np.deg2rad(2.0), min_views=2, refine=3, rigid=None,
                want_undistorted=False, as_given=False):
    """The kernel's outputs and the three margins.  `as_given` keeps float64 keypoints as they are instead of rounding them to the
    float32 the kernel reads: for the tests of the rule itself, which ask for more than float32 pixels give."""
    kp32 = np.asarray(keypoints, dtype=np.float32)
    cams = np.asarray(cams, dtype=np.float64)
    V, N, J = kp32.shape[:3]
    assert 2 <= V <= MAX_VIEWS and cams.shape == (V, CAM) and 2 <= min_views <= V
    P = N * J
    kp = (np.asarray(keypoints, dtype=np.float64) if as_given else kp32.astype(np.float64)).reshape(V, P, 3)
    sin_min = np.sin(min_angle_rad)
    with np.errstate(all='ignore'):
        S = observed(kp, conf_min)                                         # [V,P]
        a, b = undistort(cams, kp[..., 0], kp[..., 1])
        c = kp[..., 2]
        und = None
        if want_undistorted:
            und = kp32.reshape(V, P, 3).copy()
            ux, uy = _col(cams, 12, a) * a + _col(cams, 14, a), _col(cams, 13, b) * b + _col(cams, 15, b)
            und[..., 0] = np.where(S, ux.astype(np.float32), und[..., 0])
            und[..., 1] = np.where(S, uy.astype(np.float32), und[..., 1])
            und = und.reshape(V, N, J, 3)
        o, d = rays(cams, a, b)
        ob = np.broadcast_to(o[:, None, :], d.shape)
        # rule 2
        v1, v2 = pairs_of(V)
        Q = len(v1)
        both = S[v1] & S[v2]                                               # [Q,P]
        cr = np.cross(d[v1], d[v2])
        sn = np.sqrt((cr * cr).sum(-1))
        valid = both & ~(sn < sin_min)
        one = np.ones((Q, P))
        A1, b1 = ray_terms(one, ob[v1], d[v1])
        A2, b2 = ray_terms(one, ob[v2], d[v2])
        Xq, _ = solve3(A1 + A2, b1 + b2)                                   # [Q,P,3]
        e = np.full((Q, P, V), np.inf)
        e2 = np.full((Q, P, V), np.inf)
        for v in range(V):
            _, e2v = residual(cams[v], Xq, a[v][None], b[v][None])
            e2[..., v] = e2v
            e[..., v] = np.sqrt(e2v)
        scored = valid[..., None] & S.T[None]                              # [Q,P,V]
        inl = scored & (e <= tau_px)
        n = inl.sum(-1)
        cost = np.zeros((Q, P))
        for v in range(V):
            cost = cost + np.where(inl[..., v], c[v][None] * e2[..., v], 0.0)
        ar = np.arange(Q)[:, None]
        cand = valid & np.take_along_axis(inl, v1[:, None, None].repeat(P, 1), -1)[..., 0] & \
            np.take_along_axis(inl, v2[:, None, None].repeat(P, 1), -1)[..., 0]
        n_c = np.where(cand, n, 0)
        n_max = n_c.max(0)
        at = cand & (n_c == n_max[None])
        cost_c = np.where(at, cost, np.inf)
        c_min = cost_c.min(0)
        q_min = np.argmax(at & (cost_c == c_min[None]), 0)
        has = (n_max >= 2) & (n_max >= min_views)
        others = np.where(ar == q_min[None], np.inf, cost_c).min(0)
        margin_cost = np.where(has & np.isfinite(others), (others - c_min) / np.maximum(np.abs(others), 1e-300), np.inf)
        margin_tau = np.where(scored, np.abs(e - tau_px), np.inf).min((0, 2))
        margin_angle = np.where(both, np.abs(sn - sin_min), np.inf).min(0)
        mask_b = inl[q_min, np.arange(P)].T & has[None]                    # [V,P]
        # rule 4
        w = np.where(mask_b, c, 0.0)
        A = np.zeros((P, 6))
        rhs = np.zeros((P, 3))
        for v in range(V):
            Av, bv = ray_terms(w[v], ob[v], d[v])
            A += np.where(mask_b[v][:, None], Av, 0.0)
            rhs += np.where(mask_b[v][:, None], bv, 0.0)
        X0, _ = solve3(A, rhs)
        sum_c = w.sum(0)
        X = X0.copy()
        E0 = E = None
        for it in range(refine + 1):
            E = np.zeros(P)
            H = np.zeros((P, 6))
            g = np.zeros((P, 3))
            for v in range(V):
                r, e2v, Jv = residual(cams[v], X, a[v], b[v], with_j=True)
                m = mask_b[v]
                E += np.where(m, w[v] * e2v, 0.0)
                H += np.where(m[:, None], _normal(Jv, w[v]), 0.0)
                g += np.where(m[:, None], w[v][:, None] * (Jv[..., 0, :] * r[..., :1] + Jv[..., 1, :] * r[..., 1:]), 0.0)
            if it == 0:
                E0 = E
            if it == refine:
                break
            dX, _ = solve3(H, g)
            X = X - dX
        back = ~np.isfinite(E) | (E > E0)
        E = np.where(back, E0, E)
        X = np.where(back[:, None], X0, X)
        Hs = np.zeros((P, 6))
        for v in range(V):
            _, _, Jv = residual(cams[v], X, a[v], b[v], with_j=True)
            Hs += np.where(mask_b[v][:, None], _normal(Jv, np.ones(P)), 0.0)
        _, tr = solve3(Hs, np.zeros((P, 3)))
        sigma = np.sqrt(tr)
        # rules 3 and 5
        Y = X
        if rigid is not None:
            rg = np.asarray(rigid, dtype=np.float64).reshape(12)
            Y = X @ rg[:9].reshape(3, 3).T + rg[9:]
        joints = np.where(has[:, None], Y, np.nan)
        conf = np.where(has, sum_c / np.maximum(n_max, 1), 0.0).astype(np.float32)
        report = np.stack([np.where(has, n_max, 0).astype(np.float64), np.where(has, np.sqrt(E / sum_c), np.nan), np.where(has, sigma, np.nan),
                           S.sum(0).astype(np.float64)], -1)
        bits = (mask_b.astype(np.uint32) << np.arange(V, dtype=np.uint32)[:, None]).sum(0).astype(np.uint32)
    return {'joints': joints.reshape(N, J, 3), 'conf': conf.reshape(N, J), 'report': report.reshape(N, J, 4), 'inliers': bits.reshape(N, J),
            'keypoints_und': und, 'margin_tau': margin_tau.reshape(N, J), 'margin_angle': margin_angle.reshape(N, J),
            'margin_cost': margin_cost.reshape(N, J)}


def margins_ok(res, tau=1e-6, angle=1e-9, cost=1e-9):
    """The condition the equality of the discrete outputs rests on -> the points that violate it."""
    return np.argwhere((res['margin_tau'] < tau) | (res['margin_angle'] < angle) | (res['margin_cost'] < cost))


# ---- rohm_mv_residuals -----------------------------------------------------------------------------------------------------------
def view_residuals(joints_world, keypoints, cams, conf_min=0.2):
    kp32 = np.asarray(keypoints, dtype=np.float32)
    cams = np.asarray(cams, dtype=np.float64)
    V, N, J = kp32.shape[:3]
    kp = kp32.astype(np.float64).reshape(V, N * J, 3)
    X = np.asarray(joints_world, dtype=np.float64).reshape(N * J, 3)
    out = np.full((V, N * J), np.nan)
    with np.errstate(all='ignore'):
        S = observed(kp, conf_min) & np.isfinite(X).all(-1)[None]
        for v in range(V):
            R, t = cams[v, :9].reshape(3, 3), cams[v, 9:12]
            xc, yc, zc = (X @ R[k] + t[k] for k in range(3))
            px, py = distort(cams[v:v + 1], (xc / zc)[None], (yc / zc)[None])
            ex, ey = px[0] - kp[v, :, 0], py[0] - kp[v, :, 1]
            out[v] = np.where(S[v] & (zc > 0.0), np.sqrt(ex * ex + ey * ey), np.nan)
    return out.reshape(V, N, J)


# ---- the two as `rohm_amd.multiview.triangulate` / `view_residuals` on CPU tensors ---------------------------------------------------
def torch_triangulate(keypoints, cams, conf_min=0.2, tau_px=10.0, min_angle_deg=2.0, min_views=2, refine=3, rigid=None, want_undistorted=False):
    import torch
    from rohm_amd.multiview import Triangulation
    r = triangulate(keypoints.numpy(), cams.numpy(), conf_min, tau_px, np.deg2rad(min_angle_deg), min_views, refine,
                    None if rigid is None else rigid.numpy(), want_undistorted)
    return Triangulation(joints=torch.from_numpy(r['joints']), conf=torch.from_numpy(r['conf']), report=torch.from_numpy(r['report']),
                         inliers=torch.from_numpy(r["inliers"].astype(np.int32)),
                         keypoints_und=None if r['keypoints_und'] is None else torch.from_numpy(r['keypoints_und']))


def torch_view_residuals(joints_world, keypoints, cams, conf_min=0.2):
    import torch
    return torch.from_numpy(view_residuals(joints_world.numpy(), keypoints.numpy(), cams.numpy(), conf_min))


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
DISTORTION = (-0.12, 0.05, 0.001, -0.0008, -0.01)      # a moderate wide-angle lens, of a Kinect colour camera's order


def make_rig(V, seed, distortion=False, radius=4.0, focal=1000.0, arc_deg=300.0, target=(0.0, 0.0, 1.0)):
    """V cameras on an arc of `arc_deg` about `target` at `radius` metres, looking at it, z up in the world -> (camera_mtx
    [V,3,3], world2cam [V,4,4], dist_coeffs [V,5] or None)."""
    g = np.random.Generator(np.random.PCG64(seed))
    K = np.zeros((V, 3, 3))
    W = np.zeros((V, 4, 4))
    for v in range(V):
        phi = np.deg2rad(arc_deg) * v / V + g.uniform(-0.05, 0.05)
        C = np.array(target) + radius * np.array([np.cos(phi), np.sin(phi), 0.0]) + np.array([0.0, 0.0, g.uniform(0.3, 1.2)])
        z = np.array(target) + g.uniform(-0.1, 0.1, 3) - C
        z /= np.linalg.norm(z)
        x = np.cross(z, np.array([0.0, 0.0, 1.0]))
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        R = np.stack([x, y, z])
        W[v, :3, :3], W[v, :3, 3], W[v, 3, 3] = R, -R @ C, 1.0
        f = focal * g.uniform(0.97, 1.03)
        K[v] = [[f, 0.0, 640.0 + g.uniform(-8, 8)], [0.0, f * g.uniform(0.995, 1.005), 360.0 + g.uniform(-8, 8)], [0.0, 0.0, 1.0]]
    dist = None
    if distortion:
        dist = np.array(DISTORTION)[None] * g.uniform(0.7, 1.3, (V, 5))
    return K, W, dist


def project(cams, X):
    """World points X [P,3] -> distorted pixels [V,P,2] and depth [V,P]."""
    R, t = cams[:, :9].reshape(-1, 3, 3), cams[:, 9:12]
    xc = np.einsum('vij,pj->vpi', R, X) + t[:, None]
    px, py = distort(cams, xc[..., 0] / xc[..., 2], xc[..., 1] / xc[..., 2])
    return np.stack([px, py], -1), xc[..., 2]


def make_views(cams, N, J, seed, noise_px=2.0, spread=0.6, centre=(0.0, 0.0, 1.0)):
    """Random points about `centre` seen by every camera with Gaussian pixel noise and confidences in [0.5, 1] -> (keypoints
    [V,N,J,3] float32, X [N,J,3])."""
    g = np.random.Generator(np.random.PCG64(seed))
    V = cams.shape[0]
    X = np.array(centre) + g.uniform(-spread, spread, (N * J, 3))
    px, _ = project(cams, X)
    px = px + g.standard_normal(px.shape) * noise_px
    kp = np.concatenate([px, g.uniform(0.5, 1.0, (V, N * J, 1))], -1).astype(np.float32)
    return kp.reshape(V, N, J, 3), X.reshape(N, J, 3)


def plant_outliers(kp, views_per_point, seed, lo=60.0, hi=300.0):
    """Move the detection of `views_per_point` random views of every point by `lo`..`hi` px in a random direction -> (keypoints,
    planted [V,N,J] bool)."""
    g = np.random.Generator(np.random.PCG64(seed))
    V, N, J = kp.shape[:3]
    kp = kp.copy()
    planted = np.zeros((V, N, J), bool)
    for n in range(N):
        for j in range(J):
            for v in g.choice(V, views_per_point, replace=False):
                ang, rad = g.uniform(0, 2 * np.pi), g.uniform(lo, hi)
                kp[v, n, j, 0] += np.float32(rad * np.cos(ang))
                kp[v, n, j, 1] += np.float32(rad * np.sin(ang))
                planted[v, n, j] = True
    return kp, planted


def salt(kp, seed):
    """The inputs the no-result rule is about, scattered over a copy of kp [V,N,J,3]: NaN and infinite coordinates, zero, negative
    and NaN confidences, and (when N >= 3) frame 1 wholly unobserved."""
    g = np.random.Generator(np.random.PCG64(seed))
    V, N, J = kp.shape[:3]
    kp = kp.copy()
    flat = kp.reshape(-1, 3)
    M = flat.shape[0]
    k = max(1, M // 12)
    flat[g.choice(M, k, replace=False), 0] = np.nan
    flat[g.choice(M, max(1, k // 4), replace=False), 1] = np.inf
    flat[g.choice(M, k, replace=False), 2] = 0.0
    flat[g.choice(M, max(1, k // 2), replace=False), 2] = -0.5
    flat[g.choice(M, max(1, k // 2), replace=False), 2] = np.nan
    flat[g.choice(M, max(1, k // 2), replace=False), 2] = 0.1
    if N >= 3:
        kp[:, 1, :, 2] = 0.0
    return kp


# ---- the cases tests/test_gpu_multiview.py runs, built once and shared -------------------------------------------------------------------
# name: (V, N, J, seed, distortion, rigid, keypoints_und, salted, views with a planted outlier per point, duplicate view, flipped view).
# The shapes: one pair; three; five views by three frames of BODY_25; 120 pairs, more than a wave of them; 1 750 points, a multiple
# of neither 4, 16, 64 nor 256.  The seeds are chosen so that `margins_ok` holds (tests/test_multiview_ref.py asserts it on the CPU); a
# seed that stops holding is replaced here with a comment, never skipped at run time.
GPU_CASES = {
    'one_pair': (2, 1, 22, 101, False, False, False, False, 0, None, None),
    'three_views': (3, 1, 22, 102, True, True, True, False, 0, None, None),
    'five_views_salted': (5, 3, 25, 103, True, False, True, True, 1, None, 4),
    'sixteen_views': (16, 3, 22, 104, True, True, False, True, 5, (15, 3), None),
    'many_points': (4, 70, 25, 105, True, True, True, True, 1, None, None),
    'many_points_plain': (4, 70, 25, 106, False, False, False, False, 0, None, None),
    # the two sides of the kernel's switch from 16 lanes per point (up to 15 pairs) to a wave per point
    'six_views': (6, 3, 22, 107, True, False, True, True, 2, None, None),
    'seven_views': (7, 3, 22, 108, True, True, False, True, 2, None, None),
}
_CASES = {}


def build_case(name):
    """-> {'keypoints' [V,N,J,3] float32, 'cams' [V,24], 'rigid' [12] or None, 'want_undistorted', 'X' [N,J,3], 'ref': `triangulate`'s
    result, 'ref_resid': `view_residuals` of the restatement's own world joints}; read-only, cached."""
    if name in _CASES:
        return _CASES[name]
    from rohm_amd.multiview import pack_cameras
    V, N, J, seed, distortion, with_rigid, want_und, salted, bad, twin, flipped = GPU_CASES[name]
    K, W, D = make_rig(V, seed, distortion)
    if twin is not None:                                                   # two cameras at one place: their pair proposes nothing
        K[twin[0]], W[twin[0]] = K[twin[1]], W[twin[1]]
        if D is not None:
            D[twin[0]] = D[twin[1]]
    cams = pack_cameras(K, W, D)
    kp, X = make_views(cams, N, J, seed + 1000, noise_px=2.0)              # (the twin's detections carry noise of their own)
    if flipped is not None:                                                # a camera that looks away: every point is behind it
        flip = np.diag([-1.0, 1.0, -1.0])
        W[flipped, :3, :3], W[flipped, :3, 3] = flip @ W[flipped, :3, :3], flip @ W[flipped, :3, 3]
        cams = pack_cameras(K, W, D)
    if bad:
        kp, _ = plant_outliers(kp, bad, seed + 2000)
    if salted:
        kp = salt(kp, seed + 3000)
    rigid = None
    if with_rigid:
        rigid = np.concatenate([W[V - 1, :3, :3].reshape(9), W[V - 1, :3, 3]])
    ref = triangulate(kp, cams, rigid=rigid, want_undistorted=want_und)
    world = triangulate(kp, cams)['joints'] if with_rigid else ref['joints']
    case = {'keypoints': kp, 'cams': cams, 'rigid': rigid, 'want_undistorted': want_und, 'X': X, 'ref': ref, 'world': world,
            'ref_resid': view_residuals(world, kp, cams)}
    for a in (kp, cams, X, world):
        a.setflags(write=False)
    _CASES[name] = case
    return case
