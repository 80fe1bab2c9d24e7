"""TEST INFRASTRUCTURE ONLY: a float64 numpy restatement of the track resampling rule (csrc/track.hip), of `plan_times` and
of `plan_windows` (rohm_amd/data_loaders/track.py).  No scipy in here: tests/test_track_ref.py checks the slerp against it.

The rule for one output time t:
  * i0 = last valid source frame with times_src <= t, i1 = first valid one with times_src >= t; where one side does not
    exist both are the nearest valid frame (a hold) and gap = 1; alpha = (t - t0) / (t1 - t0), 0 when i0 == i1; gap = 1
    also when t1 - t0 > max_gap.
  * alpha == 0: the parameters are source row i0's bits; outside a gap so are keypoints and mask.
  * otherwise: 22 quaternion slerps, transl / betas a + alpha (b - a) -- inside a gap too.
  * keypoints outside a gap: confidence min(c0, c1); x, y interpolated in float64, rounded to float32; a bracket with
    confidence 0 has no position: x, y from the other one, confidence 0.  mask: min(m0, m1).  Inside a gap (holds
    included): zeros."""
import numpy as np

ROT_COLS = [0] + [16 + 3 * j for j in range(21)]          # first column of the 22 rotation vectors in a [79] row


def rotvec_to_quat(rv):
    """[..., 3] -> [..., 4] (x, y, z, w), small-angle series below 1e-3 rad."""
    rv = np.asarray(rv, dtype=np.float64)
    a2 = (rv * rv).sum(-1)
    a = np.sqrt(a2)
    with np.errstate(invalid='ignore', divide='ignore'):
        sc = np.where(a <= 1e-3, 0.5 - a2 / 48.0 + a2 * a2 / 3840.0, np.sin(a / 2.0) / a)
    return np.concatenate([sc[..., None] * rv, np.cos(a / 2.0)[..., None]], axis=-1)


def quat_to_rotvec(q):
    """Normalise, w >= 0, angle = 2 atan2(|v|, w): the shortest rotation vector."""
    q = q / np.sqrt((q * q).sum(-1, keepdims=True))
    q = np.where(q[..., 3:4] < 0, -q, q)
    ang = 2.0 * np.arctan2(np.sqrt((q[..., :3] ** 2).sum(-1)), q[..., 3])
    a2 = ang * ang
    with np.errstate(invalid='ignore', divide='ignore'):
        sc = np.where(ang <= 1e-3, 2.0 + a2 / 12.0 + 7.0 * a2 * a2 / 2880.0, ang / np.sin(ang / 2.0))
    return sc[..., None] * q[..., :3]


def slerp_rotvec(r0, r1, alpha):
    """r0, r1 [..., 3] rotation vectors, alpha [...] -> [..., 3]."""
    q0, q1 = rotvec_to_quat(r0), rotvec_to_quat(r1)
    alpha = np.asarray(alpha, dtype=np.float64)
    d = (q0 * q1).sum(-1)
    q1 = np.where((d < 0)[..., None], -q1, q1)
    d = np.abs(d)
    omega = np.arctan2(np.sqrt(np.maximum(1.0 - d * d, 0.0)), d)
    so = np.sin(omega)
    lerp = so < 1e-8
    with np.errstate(invalid='ignore', divide='ignore'):
        w0 = np.where(lerp, 1.0 - alpha, np.sin((1.0 - alpha) * omega) / so)
        w1 = np.where(lerp, alpha, np.sin(alpha * omega) / so)
    return quat_to_rotvec(w0[..., None] * q0 + w1[..., None] * q1)


def rotvec_to_matrix(rv):
    q = rotvec_to_quat(rv)
    x, y, z, w = (q[..., i] for i in range(4))
    M = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                  2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=-1)
    return M.reshape(M.shape[:-1] + (3, 3))


def geodesic(ra, rb):
    """Angle (rad) of the relative rotation between rotation vectors ra, rb [..., 3]: 2 atan2(|v|, |w|) of qa^-1 qb, which
    stays accurate at angle 0 (an arccos of the trace does not)."""
    qa, qb = rotvec_to_quat(ra), rotvec_to_quat(rb)
    va, wa, vb, wb = qa[..., :3], qa[..., 3:], qb[..., :3], qb[..., 3:]
    w = wa[..., 0] * wb[..., 0] + (va * vb).sum(-1)
    v = wa * vb - wb * va - np.cross(va, vb)
    return 2.0 * np.arctan2(np.sqrt((v * v).sum(-1)), np.abs(w))


def brackets(times_src, valid, times_dst, max_gap):
    """-> i0, i1 (int64 source indices), alpha (float64), gap (bool), per output time."""
    ts, td = np.asarray(times_src, dtype=np.float64), np.asarray(times_dst, dtype=np.float64)
    vi = np.flatnonzero(np.asarray(valid, dtype=bool))
    tv = ts[vi]
    c = np.searchsorted(tv, td, side='right')              # valid frames with time <= t
    k0, k1 = c - 1, c.copy()
    exact = (k0 >= 0) & (tv[np.maximum(k0, 0)] == td)
    k1 = np.where(exact, k0, k1)
    before, after = k0 < 0, k1 >= len(vi)
    k0 = np.where(before, 0, k0)
    k1 = np.where(before, 0, np.where(after, k0, k1))
    i0, i1 = vi[k0], vi[k1]
    t0, t1 = ts[i0], ts[i1]
    with np.errstate(invalid='ignore', divide='ignore'):
        alpha = np.where(i0 == i1, 0.0, (td - t0) / (t1 - t0))
    gap = before | after | ((t1 - t0) > max_gap)
    return i0, i1, alpha, gap


def resample(times_src, valid, params, keypoints, mask_joint, times_dst, max_gap):
    """-> dict(params [n,79] float64, keypoints [n,J,3] float32 or None, mask_joint [n,M] float32 or None, src_index int32,
    gap uint8)."""
    params = np.asarray(params, dtype=np.float64)
    i0, i1, alpha, gap = brackets(times_src, valid, times_dst, max_gap)
    copy = alpha == 0.0
    p0, p1 = params[i0], params[i1]
    out = p0 + alpha[:, None] * (p1 - p0)
    for c in ROT_COLS:
        out[:, c:c + 3] = slerp_rotvec(p0[:, c:c + 3], p1[:, c:c + 3], alpha)
    out[copy] = p0[copy]
    res = {'params': out, 'keypoints': None, 'mask_joint': None, 'src_index': i0.astype(np.int32), 'gap': gap.astype(np.uint8)}
    if keypoints is not None:
        kp = np.asarray(keypoints, dtype=np.float32)
        k0, k1 = kp[i0], kp[i1]
        c0, c1 = k0[..., 2], k1[..., 2]
        xy = (k0[..., :2].astype(np.float64) + alpha[:, None, None] * (k1[..., :2].astype(np.float64) - k0[..., :2].astype(np.float64))
              ).astype(np.float32)
        xy = np.where((c1 == 0)[..., None], k0[..., :2], xy)
        xy = np.where((c0 == 0)[..., None], k1[..., :2], xy)
        conf = np.where((c0 == 0) | (c1 == 0), np.float32(0.0), np.minimum(c0, c1))
        o = np.concatenate([xy, conf[..., None]], axis=-1).astype(np.float32)
        o[copy] = k0[copy]
        o[gap] = 0.0
        res['keypoints'] = o
    if mask_joint is not None:
        m = np.asarray(mask_joint, dtype=np.float32)
        o = np.minimum(m[i0], m[i1])
        o[copy] = m[i0][copy]
        o[gap] = 0.0
        res['mask_joint'] = o
    return res


def plan_times(times_src, valid, fps_out=30.0):
    tv = np.asarray(times_src, dtype=np.float64)[np.asarray(valid, dtype=bool)]
    t0, t_last = float(tv[0]), float(tv[-1])
    n_out = int(np.floor((t_last - t0) * fps_out + 1e-9)) + 1
    return np.array([t0 + k / fps_out for k in range(n_out)], dtype=np.float64)


def plan_windows(n, clip_len, overlap_len, tail='cover'):
    if n < clip_len:
        raise ValueError(f'{n} frames are fewer than one clip of {clip_len}')
    step = clip_len - overlap_len
    starts = list(range(0, n - clip_len + 1, step))
    if tail == 'cover' and starts[-1] + clip_len < n:
        starts.append(n - clip_len)
    return starts


# ---- shared synthetic tracks ---------------------------------------------------------------------------------------------
def random_rotvecs(g, shape, max_angle):
    ax = g.standard_normal(shape + (3,))
    ax /= np.linalg.norm(ax, axis=-1, keepdims=True)
    return ax * g.uniform(0.0, max_angle, size=shape + (1,))


def compose(ra, rb):
    """Rotation vector of R(ra) R(rb)."""
    qa, qb = rotvec_to_quat(ra), rotvec_to_quat(rb)
    va, wa, vb, wb = qa[..., :3], qa[..., 3:], qb[..., :3], qb[..., 3:]
    w = wa * wb - (va * vb).sum(-1, keepdims=True)
    v = wa * vb + wb * va + np.cross(va, vb)
    return quat_to_rotvec(np.concatenate([v, w], axis=-1))


def smooth_params(g, n, step_angle=0.15, base_angle=1.0):
    """[n,79] float64 rows whose rotations stay below 3.0 rad with at most 2.0 rad between any two frames that a test may
    bracket (a random walk of `step_angle` per frame from a base of at most `base_angle`; holes of up to 6 frames)."""
    out = np.zeros((n, 79))
    for c in ROT_COLS:
        r = random_rotvecs(g, (), base_angle)
        for i in range(n):
            out[i, c:c + 3] = r
            r = compose(r, random_rotvecs(g, (), step_angle))
    out[:, 3:6] = np.cumsum(g.standard_normal((n, 3)) * 0.02, axis=0) + np.array([0.1, -0.2, 2.5])
    out[:, 6:16] = g.standard_normal(10) * 0.5 + g.standard_normal((n, 10)) * 0.01
    assert max(np.linalg.norm(out[:, c:c + 3], axis=-1).max() for c in ROT_COLS) < 3.0
    return out
