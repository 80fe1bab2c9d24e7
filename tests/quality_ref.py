"""float64 numpy restatement of csrc/quality.hip (`rohm_track_quality`, `rohm_floor_clearance`): the rule the kernels are held
to in tests/test_gpu_quality.py, itself held to hand-computable cases in tests/test_quality_ref.py.  Column layouts are in
include/rohm_hip.h.  Inputs are taken as float32 (what the kernels read) and every operation is float64."""
import numpy as np

FOOT = (7, 8, 10, 11)                    # ankles, toes
FOOT_HMAX = (0.15, 0.15, 0.10, 0.10)
TOES = (10, 11)
SPEED_MIN = 0.10
PENE_DEPTH = -0.05
N_COLS, N_TOT = 10, 15
COLS = ('reproj_px', 'reproj_max_px', 'reproj_n', 'skate', 'accel', 'pene', 'dev_vis', 'dev_occ', 'n_vis', 'gap')


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def project(joints, scene2cam, fx, fy, cx, cy):
    """scene2cam . joint and its pinhole projection -> (uv [..., 2], Z [...]) in float64."""
    j = _f32(joints)
    m = np.asarray(scene2cam, dtype=np.float64).reshape(4, 4)
    cam = j @ m[:3, :3].T + m[:3, 3]
    with np.errstate(divide='ignore', invalid='ignore'):
        uv = np.stack([fx * cam[..., 0] / cam[..., 2] + cx, fy * cam[..., 1] / cam[..., 2] + cy], axis=-1)
    return uv, cam[..., 2], cam


def _horizontal(up_axis):
    return (0, 1) if up_axis == 2 else (0, 2)


def foot_terms(joints, fps, up_axis, ground):
    """(speed [N-1, 4], height above the floor at t [N-1, 4]) of ankles 7, 8 and toes 10, 11 for the pairs (t, t + 1)."""
    j = _f32(joints)[:, FOOT]
    d = j[1:] - j[:-1]
    a, b = _horizontal(up_axis)
    speed = np.sqrt(d[..., a] ** 2 + d[..., b] ** 2) * fps
    return speed, j[:-1, :, up_axis] - ground


def track_quality(joints, fps=30.0, up_axis=2, has_floor=True, ground_height=0.0, scene2cam=None, fx=0.0, fy=0.0, cx=0.0, cy=0.0,
                  keypoints=None, conf_min=0.2, joints_ref=None, mask_ref=None, gap=None):
    """-> (rows [N, 10], totals [2, 15]) float64."""
    j = _f32(joints).reshape(-1, 22, 3)
    N = len(j)
    ground = float(np.float32(ground_height)) if has_floor else 0.0
    conf_min = float(np.float32(conf_min))
    fps = float(fps)
    rows = np.full((N, N_COLS), np.nan)
    g = np.zeros(N, np.uint8) if gap is None else (np.asarray(gap).reshape(N) != 0).astype(np.uint8)
    rows[:, 9] = g
    rows[:, 2] = 0.0
    with np.errstate(invalid='ignore', divide='ignore'):
        # reprojection
        if keypoints is not None:
            kp = _f32(keypoints).reshape(N, 22, 3)
            uv, Z, cam = project(j, scene2cam, fx, fy, cx, cy)
            conf = kp[..., 2] > conf_min
            bad = conf & ~np.isfinite(cam).all(axis=-1)
            qual = conf & ~bad & (Z > 0.0)
            d = np.sqrt(((uv - kp[..., :2]) ** 2).sum(-1))
            c = kp[..., 2]
            n = qual.sum(axis=1)
            scored = ~bad.any(axis=1) & (n > 0)
            rows[:, 2] = np.where(bad.any(axis=1), np.nan, n)
            rows[:, 0] = np.where(scored, np.where(qual, c * d, 0.0).sum(axis=1) / np.where(qual, c, 0.0).sum(axis=1), np.nan)
            rows[:, 1] = np.where(scored, np.where(qual, d, -np.inf).max(axis=1, initial=-np.inf), np.nan)
        # skating
        if has_floor and N > 1:
            speed, h = foot_terms(j, fps, up_axis, ground)
            ok = ((speed > SPEED_MIN) & (h < np.asarray(FOOT_HMAX))).all(axis=1)
            nan = (np.isnan(speed) | np.isnan(h)).any(axis=1)
            rows[:-1, 3] = np.where(nan, np.nan, ok.astype(np.float64))
        # acceleration
        if N > 2:
            a = (j[2:] - 2.0 * j[1:-1]) + j[:-2]
            rows[:-2, 4] = (np.sqrt((a ** 2).sum(-1)) * (fps * fps)).sum(-1) / 22.0
        # toes
        toe_d = j[:, TOES, up_axis] - ground
        if has_floor:
            pen = np.where(toe_d < 0.0, toe_d, np.where(np.isnan(toe_d), toe_d, 0.0))
            rows[:, 5] = np.where(np.isnan(pen).any(axis=1), np.nan, pen.min(axis=1))
        # distance to the input track
        mk = np.ones((N, 22)) if mask_ref is None else _f32(mask_ref).reshape(N, 22)
        vis, occ = mk == 1.0, mk == 0.0
        rows[:, 8] = vis.sum(axis=1)
        if joints_ref is not None:
            dev = np.sqrt(((j - _f32(joints_ref).reshape(N, 22, 3)) ** 2).sum(-1))
            for col, sel in ((6, vis), (7, occ)):
                rows[:, col] = np.where(sel.any(axis=1), np.where(sel, dev, 0.0).sum(axis=1) / sel.sum(axis=1), np.nan)
    return rows, totals_from(rows, toe_d if has_floor else None)


def totals_from(rows, toe_d=None):
    """totals [2, 15] from the rows and, for columns 8 .. 10, the toe heights above the floor [N, 2] (None: no floor)."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, N_COLS)
    tot = np.zeros((2, N_TOT))
    for g in (0, 1):
        sel = rows[:, 9] == g
        r = rows[sel]
        tot[g, 0] = len(r)
        for col, s, n in ((0, 1, 2), (3, 4, 5), (4, 6, 7), (6, 11, 12), (7, 13, 14)):
            v = r[:, col]
            v = v[~np.isnan(v)]
            tot[g, s], tot[g, n] = v.sum(), len(v)
        m = r[~np.isnan(r[:, 0]), 1]
        tot[g, 3] = np.nan if len(m) == 0 else (np.nan if np.isnan(m).any() else m.max())
        if toe_d is not None:
            d = np.asarray(toe_d, dtype=np.float64)[sel].reshape(-1)
            d = d[~np.isnan(d)]
            tot[g, 8], tot[g, 9], tot[g, 10] = (d < PENE_DEPTH).sum(), np.minimum(d, 0.0).sum(), len(d)
    return tot


def threshold_margin(joints, fps, up_axis, ground_height, scene2cam=None):
    """The least distance of any compared quantity from its threshold: foot speeds from 0.10 m/s, foot heights from 0.15 /
    0.10 m, toe heights from -0.05 m and camera depths from 0 -- flags and counts can be compared exactly when it is large
    against the rounding of the compared quantities.  NaN entries are left out."""
    j = _f32(joints).reshape(-1, 22, 3)
    ground = float(np.float32(ground_height))
    parts = [np.abs(j[:, TOES, up_axis] - ground - PENE_DEPTH).reshape(-1)]
    if len(j) > 1:
        speed, h = foot_terms(j, float(fps), up_axis, ground)
        parts += [np.abs(speed - SPEED_MIN).reshape(-1), np.abs(h - np.asarray(FOOT_HMAX)).reshape(-1)]
    if scene2cam is not None:
        parts.append(np.abs(project(j, scene2cam, 1.0, 1.0, 0.0, 0.0)[1]).reshape(-1))
    v = np.concatenate(parts)
    v = v[~np.isnan(v)]
    return float(v.min()) if v.size else np.inf


def floor_clearance(verts, up_axis, ground_height, below=0.05):
    """-> [n, 3] float64: lowest vertex height above the floor, its index (the lowest on ties), vertices more than `below`
    under the floor; (NaN, -1, NaN) for a frame with a vertex height that is not finite."""
    h = _f32(verts)[..., up_axis] - float(np.float32(ground_height))
    out = np.stack([h.min(axis=1), h.argmin(axis=1).astype(np.float64), (h < -float(np.float32(below))).sum(axis=1).astype(np.float64)], axis=1)
    out[~np.isfinite(h).all(axis=1)] = (np.nan, -1.0, np.nan)
    return out
