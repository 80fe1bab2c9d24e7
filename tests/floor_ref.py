"""float64 numpy restatement of csrc/floor.hip (`rohm_floor_candidates`, `rohm_floor_hypotheses`, `rohm_floor_moments`) and of
`rohm_amd.floor.estimate_floor`: the rule the kernels and the estimator are held to in tests/test_gpu_floor.py, itself held to
hand-computable cases in tests/test_floor_ref.py.  The rules are stated in include/rohm_hip.h and in rohm_amd/floor.py.  Inputs
are taken as float32 (what the kernels read) and every operation is float64.  The refinement and the camera pose are written
out again here, not imported; only `FloorEstimate` and the refusals (`check_candidates`, `check_estimate`) are the module's."""
import numpy as np

import helpers

TOES = (10, 11)
SIGMA = 0.005                    # the noise of the noisy planted floor: 5 mm
record = helpers.parity_recorder('floor_parity.json')
DEGENERATE = 1e-9
INT64_MIN = np.iinfo(np.int64).min
UP = {'z': 2, 'y': 1}


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


# ---- rohm_floor_candidates ---------------------------------------------------------------------------------------------------
def candidate_terms(joints, times, valid_idx):
    """(i [Nv-1], dt [Nv-1], speed [Nv-1, 2]) of every valid frame that has a successor in valid_idx."""
    j = _f32(joints).reshape(-1, 22, 3)[:, TOES]
    t = np.asarray(times, dtype=np.float64).reshape(-1)
    vi = np.asarray(valid_idx, dtype=np.int64).reshape(-1)
    i, i2 = vi[:-1], vi[1:]
    dt = t[i2] - t[i]
    d = j[i2] - j[i]
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        speed = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]) / dt[:, None]
    return i, dt, speed


def candidates(joints, times, valid_idx, keypoints=None, conf_min=0.2, v_max=0.10, max_gap=0.05):
    """-> flags [N, 2] uint8."""
    N = len(np.asarray(joints).reshape(-1, 22, 3))
    flags = np.zeros((N, 2), np.uint8)
    if len(np.asarray(valid_idx).reshape(-1)) < 2:
        return flags
    i, dt, speed = candidate_terms(joints, times, valid_idx)
    with np.errstate(invalid='ignore'):
        rest = ((dt > 0.0) & (dt <= float(max_gap)))[:, None] & (speed < float(v_max))
        if keypoints is not None:
            conf = _f32(keypoints).reshape(N, 22, 3)[:, TOES, 2]
            rest = rest & (conf[i] > float(np.float32(conf_min)))
    flags[i] = rest.astype(np.uint8)
    return flags


def candidate_points(joints, flags):
    """The flagged toe positions [P, 3] float32, frame-major, toe 10 before toe 11: the wrapper's compaction."""
    toes = np.asarray(joints, dtype=np.float32).reshape(-1, 22, 3)[:, TOES].reshape(-1, 3)
    return toes[np.flatnonzero(np.asarray(flags).reshape(-1))]


# ---- rohm_floor_hypotheses -----------------------------------------------------------------------------------------------------
def triple_planes(points, triples):
    """(planes [K, 4] with NaN rows for degenerate triples, live [K] bool)."""
    p = _f32(points).reshape(-1, 3)[np.asarray(triples, dtype=np.int64).reshape(-1, 3)]
    u, v = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        n = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)
        length = np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])
        live = (length >= DEGENERATE) & np.isfinite(length)
        n = n / length[:, None]
        d = -(n[:, 0] * p[:, 0, 0] + n[:, 1] * p[:, 0, 1] + n[:, 2] * p[:, 0, 2])
    planes = np.concatenate([n, d[:, None]], axis=1)
    planes[~live] = np.nan
    return planes, live


def _signed(planes, x):
    """[K, n] signed distances of the positions x [n, 3] to the planes [K, 4]."""
    with np.errstate(invalid='ignore', over='ignore'):
        return planes[:, 0:1] * x[None, :, 0] + planes[:, 1:2] * x[None, :, 1] + planes[:, 2:3] * x[None, :, 2] + planes[:, 3:4]


def hypotheses(points, joints, triples, tau=0.03, under_tol=0.08, chunk=64, margins=False):
    """-> (planes [K, 4] float64, scores [K, 3] int64, best int); with margins=True also margin [K]: how close any compared
    distance of hypothesis h comes to tau or under_tol (inf for a degenerate triple)."""
    pts, jts = _f32(points).reshape(-1, 3), _f32(joints).reshape(-1, 3)
    planes, live = triple_planes(pts, triples)
    K = len(planes)
    scores = np.zeros((K, 3), np.int64)
    margin = np.full(K, np.inf)
    for a in range(0, K, chunk):
        pl = planes[a:a + chunk]
        s = _signed(pl, jts)
        with np.errstate(invalid='ignore'):
            pos, neg = (s > under_tol).sum(axis=1), (s < -under_tol).sum(axis=1)
        flip = neg > pos
        pl[flip] = -pl[flip]
        under = np.where(flip, pos, neg)
        r = _signed(pl, pts)
        with np.errstate(invalid='ignore'):
            support = (np.abs(r) <= tau).sum(axis=1)
        scores[a:a + chunk] = np.stack([support - under, support, under], axis=1)
        if margins:
            with np.errstate(invalid='ignore'):
                ms = np.abs(np.abs(s) - under_tol)
                mr = np.abs(np.abs(r) - tau)
                margin[a:a + chunk] = np.minimum(np.nanmin(ms, axis=1, initial=np.inf), np.nanmin(mr, axis=1, initial=np.inf))
    scores[~live] = (INT64_MIN, 0, 0)
    margin[~live] = np.inf
    best = int(np.argmax(scores[:, 0])) if live.any() else -1           # argmax: the lowest index on ties
    return (planes, scores, best, margin) if margins else (planes, scores, best)


_hypotheses = hypotheses      # `estimate_floor` has an option of that name


# ---- rohm_floor_moments ----------------------------------------------------------------------------------------------------------
def moments(points, plane, origin, tau=0.03):
    """-> out [11] float64."""
    p = _f32(points).reshape(-1, 3)
    pl, o = np.asarray(plane, dtype=np.float64).reshape(4), np.asarray(origin, dtype=np.float64).reshape(3)
    with np.errstate(invalid='ignore'):
        r = p[:, 0] * pl[0] + p[:, 1] * pl[1] + p[:, 2] * pl[2] + pl[3]
        inl = np.abs(r) <= tau
    q, r = p[inl] - o, r[inl]
    return np.array([inl.sum(), q[:, 0].sum(), q[:, 1].sum(), q[:, 2].sum(), (q[:, 0] * q[:, 0]).sum(), (q[:, 0] * q[:, 1]).sum(),
                     (q[:, 0] * q[:, 2]).sum(), (q[:, 1] * q[:, 1]).sum(), (q[:, 1] * q[:, 2]).sum(), (q[:, 2] * q[:, 2]).sum(),
                     (r * r).sum()], dtype=np.float64)


# ---- estimate_floor ----------------------------------------------------------------------------------------------------------------
def fit(m, origin, n_prev):
    cnt = m[0]
    mean = m[1:4] / cnt
    cov = np.array([[m[4], m[5], m[6]], [m[5], m[7], m[8]], [m[6], m[8], m[9]]]) / cnt - mean[:, None] * mean[None, :]
    w, v = np.linalg.eigh(cov)
    n = v[:, 0] * (-1.0 if v[:, 0] @ n_prev < 0 else 1.0)
    c = origin + mean
    return n, -(n @ c), c, w


def pose(n, d, up_axis):
    e = np.eye(3)[UP[up_axis]]
    c = n @ e
    if c < -1.0 + 1e-12:
        a = np.cross(e, np.eye(3)[0])
        if np.linalg.norm(a) < 0.5:
            a = np.cross(e, np.eye(3)[1])
        a = a / np.linalg.norm(a)
        R = 2.0 * a[:, None] * a[None, :] - np.eye(3)
    else:
        v = np.cross(n, e)
        vx = np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])
        R = np.eye(3) + vx + vx @ vx / (1.0 + c)
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, d * e
    return M


def estimate_floor(joints, times=None, valid=None, keypoints=None, fps=30.0, up_axis='z', tau=0.03, under_tol=0.08, v_max=0.10,
                   max_gap=None, conf_min=0.2, hypotheses=4096, seed=0, refine=2, toe_height=0.0, min_candidates=30, min_support=0.5,
                   min_extent=0.10, strict=True):
    """`rohm_amd.floor.estimate_floor` on host arrays -> FloorEstimate."""
    from rohm_amd.floor import FloorEstimate, check_candidates, check_estimate
    if up_axis not in UP:
        raise ValueError(f"up_axis must be 'z' or 'y', got {up_axis!r}")
    j = np.asarray(joints, dtype=np.float32).reshape(-1, 22, 3)
    N = len(j)
    ts = np.arange(N, dtype=np.float64) / float(fps) if times is None else np.asarray(times, dtype=np.float64).reshape(N)
    v = np.ones(N, bool) if valid is None else np.asarray(valid).astype(bool).reshape(N)
    if max_gap is None:
        max_gap = float(1.5 * np.median(np.diff(ts))) if N > 1 else 0.0
    vi = np.flatnonzero(v)
    points = candidate_points(j, candidates(j, ts, vi, keypoints, conf_min, v_max, max_gap))
    P = len(points)
    check_candidates(P, min_candidates, strict)
    triples = np.random.Generator(np.random.PCG64(seed)).integers(0, P, size=(int(hypotheses), 3)).astype(np.int32)
    planes, scores, best = _hypotheses(points, j[vi].reshape(-1, 3), triples, tau, under_tol)
    if best < 0:
        raise ValueError(f'all {int(hypotheses)} triples of contacts are degenerate (hypotheses={int(hypotheses)}): the contacts are on one line')
    origin = points[triples[best]].astype(np.float64).mean(axis=0)
    n, d = planes[best, :3], float(planes[best, 3])
    for _ in range(int(refine)):
        m = moments(points, np.append(n, d), origin, tau)
        if m[0] < 3:
            break
        n, d, _, _ = fit(m, origin, n)
    m = moments(points, np.append(n, d), origin, tau)
    support = int(m[0])
    _, _, centroid, w = fit(m, origin, n) if support > 0 else (None, None, np.full(3, np.nan), np.zeros(3))
    est = FloorEstimate(normal=n, offset=float(d), cam2world=pose(n, d, up_axis), floor_height=0.0 - float(toe_height), candidates=P, support=support,
                        under=int(scores[best, 2]), rms=float(np.sqrt(m[10] / m[0])) if support else float('nan'),
                        extent=float(np.sqrt(max(w[1], 0.0))), hypothesis=best, tilt_deg=float(np.degrees(np.arccos(np.clip(-n[1], -1.0, 1.0)))),
                        centroid=centroid, up_axis=up_axis)
    if strict:
        check_estimate(est, min_support, min_extent)
    return est


# ---- planted floors (shared by the CPU and the GPU tests) ----------------------------------------------------------------------------
SLOPE = (0.25, -0.5, 3.0)        # the planted floor z = 0.25 x - 0.5 y + 3 in a y-down camera looking along z: dyadic, see below


def planted_plane():
    """(n, d) of the planted floor, n towards the body (towards the camera's -y side)."""
    a, b, c = SLOPE
    n = np.array([a, b, -1.0])
    n = n / np.linalg.norm(n)
    return n, float(-n @ np.array([0.0, 0.0, c]))


def planted_track(stances=200, sigma=0.0, step_share=0.2, seed=0):
    """A walk over the planted floor: per stance two frames in which each toe keeps its position exactly (speed 0: at rest in
    the first frame of the pair), then a jump of decimetres to the next stance (tens of m/s: not at rest).  Contact positions
    have x, y on a grid of 1 / 256 m inside a 2 m x 1 m patch; with the dyadic slopes of `SLOPE` their z is exact in float32, so
    with sigma = 0 the float32 track holds points *on* the plane and the planted plane can be recovered to float64 rounding.
    `step_share` of the stances stand on a second plane 0.4 m higher (a step); sigma is Gaussian noise along the normal, one
    draw per contact.  The other 20 joints are 0.3 .. 1.9 m above their stance's toes.  -> (joints [2 * stances, 22, 3]
    float32, on_floor [stances] bool)."""
    g = np.random.Generator(np.random.PCG64(seed))
    n, _ = planted_plane()
    a, b, c = SLOPE
    xy = np.stack([g.integers(-256, 257, size=(stances, 2)) / 256.0, g.integers(-128, 129, size=(stances, 2)) / 256.0], axis=-1)     # [S, toe, (x, y)]
    toes = np.concatenate([xy, (a * xy[..., 0] + b * xy[..., 1] + c)[..., None]], axis=-1)
    on_floor = g.uniform(size=stances) >= step_share
    toes = toes + np.where(on_floor, 0.0, 0.4)[:, None, None] * n
    if sigma > 0:
        toes = toes + g.normal(0.0, sigma, size=(stances, 2, 1)) * n
    body = toes.mean(axis=1, keepdims=True) + g.uniform(0.5, 1.7, size=(stances, 20, 1)) * n + g.uniform(-0.1, 0.1, size=(stances, 20, 3))
    j = np.zeros((stances, 22, 3))
    j[:, list(TOES)] = toes
    j[:, [k for k in range(22) if k not in TOES]] = body
    return np.repeat(j, 2, axis=0).astype(np.float32), on_floor


def plane_errors(est):
    """(angle in radians between the estimate's normal and the planted one, distance of the estimate's centroid to the planted
    plane): the two quantities whose first-order standard errors are sigma / (extent sqrt(support)) and sigma / sqrt(support)."""
    n, d = planted_plane()
    angle = float(np.arctan2(np.linalg.norm(np.cross(n, est.normal)), n @ est.normal))
    return angle, abs(float(n @ est.centroid + d))
