"""TEST INFRASTRUCTURE ONLY: float64 numpy restatements of the clip-side work of the reference's test-time loader
(data_loaders/dataloader_video.py:373-403, :441-484): the two canonicalisations (data_loaders/motion_representation.py
:47-184), the keypoint undistortion with its forward model, and the visibility-mask rule.  The motion representation
itself is oracle/rederive.py::get_repr_smplx.  Pinned to the reference's own functions by tests/golden/clips.npz
(scripts/make_golden_clips.py); the undistortion arithmetic is NOT pinned (cv2 is absent where the fixtures are made)
and follows OpenCV's documented algorithm."""
import math

import numpy as np

from oracle import frames as OF
from oracle import geometry as G
from oracle import rederive as RD

R_HIP, L_HIP, SDR_R, SDR_L = 2, 1, 17, 16          # as cano_seq_smplx unpacks face_joint_indx
# the inputs of tests/golden/clips.npz (scripts/make_golden_clips.py)
CLIP_SEED, CLIP_N, CLIP_L, CLIP_OVERLAP = 5, 48, 16, 2
DEGENERATE_FRAMES = (5, 9)
PARAM_COLS = {'global_orient': (0, 3), 'transl': (3, 6), 'betas': (6, 16), 'body_pose': (16, 79)}


def clip_preset(joints_world, up_axis):
    """The preset floor of the fixture's 'preset' cases: 2 cm under the recording's lowest joint."""
    return float(joints_world[:, :, {'z': 2, 'y': 1}[up_axis]].min()) - 0.02


def split_world(world):
    return {k: world[:, a:b] for k, (a, b) in PARAM_COLS.items()}


def _unit(v):
    return v / np.sqrt((v * v).sum())


def canonicalize(positions, params, up_axis='z', preset_floor_height=None):
    """positions [T,22,3] float32 (scene coordinates), params: dict of float64 arrays.  Returns canonical joints
    [T,22,3] float64 (z up, frame 0 at the xy origin facing +y, feet on the floor), canonical params, transf [4,4]."""
    up = {'z': 2, 'y': 1}[up_axis]
    pos32 = np.array(positions, dtype=np.float32)
    # a falsy preset (None or 0.0) means "take the lowest joint"; the subtraction stays in float32
    floor = preset_floor_height if preset_floor_height else pos32[:, :, up].min()
    pos32[:, :, up] -= np.float32(floor)
    origin = pos32[0, 0].astype(np.float64)
    origin[up] = 0.0
    pos = pos32.astype(np.float64) - origin
    x = (pos[0, R_HIP] - pos[0, L_HIP]) + (pos[0, SDR_R] - pos[0, SDR_L])
    x[up] = 0.0
    x = _unit(x)
    e_up = np.zeros(3)
    e_up[up] = 1.0
    y = _unit(np.cross(e_up, x))
    if up_axis == 'z':
        rot = np.stack([x, y, e_up])                                  # rows: new x, y, z axes in scene coordinates
    else:
        first = -np.stack([x, e_up, y])                               # y down after this ...
        rx = np.array([[1, 0, 0], [0, math.cos(-math.pi / 2), -math.sin(-math.pi / 2)],
                       [0, math.sin(-math.pi / 2), math.cos(-math.pi / 2)]])
        rz = np.array([[math.cos(math.pi), -math.sin(math.pi), 0], [math.sin(math.pi), math.cos(math.pi), 0], [0, 0, 1]])
        rot = rz @ rx @ first                                         # ... then z up
    shift = -origin
    shift[up] = -float(floor)
    transf = np.eye(4)
    transf[:3, :3] = rot
    transf[:3, 3] = rot @ shift
    cano = pos @ rot.T
    delta = np.asarray(positions)[:, 0] - params['transl']
    go, tr = OF.update_global_rt(params['global_orient'], params['transl'], delta, transf)
    new = dict(params)
    new['global_orient'], new['transl'] = go, tr
    return cano, new, transf


def window_starts(n_frames, clip_len, overlap):
    out, c = [], 0
    while c * (clip_len - overlap) + clip_len <= n_frames:
        out.append(c * (clip_len - overlap))
        c += 1
    return out


def build_clips(joints_world, smplx_world, clip_len, overlap_len=2, up_axis='z', preset_floor_height=None, stats=None,
                starts=None, all_f64=False):
    """What `create_body_repr` + the normalisation of `__getitem__` produce for every clip, stacked (float64)."""
    if starts is None:
        starts = window_starts(len(joints_world), clip_len, overlap_len)
    out = {k: [] for k in ('repr', 'cano_joints', 'global_orient', 'transl', 'transf_matrix')}
    for s in starts:
        pos = joints_world[s:s + clip_len]
        prm = split_world(smplx_world[s:s + clip_len])
        cano, cp, tm = canonicalize(pos, prm, up_axis, preset_floor_height)
        full = RD.full_repr((get_repr_f64 if all_f64 else RD.get_repr_smplx)(cano, cp))
        if stats is not None:
            full = (full - stats[0]) / stats[1]
        out['repr'].append(full)
        out['cano_joints'].append(cano)
        out['global_orient'].append(cp['global_orient'])
        out['transl'].append(cp['transl'])
        out['transf_matrix'].append(tm)
    L = clip_len
    shapes = {'repr': (0, L - 1, 294), 'cano_joints': (0, L, 22, 3), 'global_orient': (0, L, 3), 'transl': (0, L, 3),
              'transf_matrix': (0, 4, 4)}
    res = {k: (np.stack(v) if v else np.zeros(shapes[k])) for k, v in out.items()}
    res['starts'] = np.asarray(starts, dtype=np.int64)
    return res


def get_repr_f64(positions, params):
    """The representation with the quaternion algebra in float64 too (for measuring how far the reference's float32
    flow is from exact arithmetic; not a reference of anything)."""
    import unittest.mock as mock
    import torch
    with mock.patch.object(RD, '_f32', lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()), \
            mock.patch.object(RD, '_qinv', lambda q: np.asarray(q, np.float64) * np.array([1., -1., -1., -1.])):
        return RD.get_repr_smplx(positions, params)


# PROX-like colour-camera intrinsics and (k1, k2, p1, p2, k3) (the Kinect colour camera of PROX is of this kind)
PROX_K = np.array([[1060.531764702488, 0, 951.2999547224418], [0, 1060.3856705041237, 536.7703598373467], [0, 0, 1.0]])
PROX_DIST = np.array([0.05, -0.04, 0.001, -0.0008, 0.01])


# ---- keypoints ---------------------------------------------------------------------------------------------------------
def distort_normalized(x, y, k):
    """OpenCV's forward model for (k1, k2, p1, p2, k3) on normalised image coordinates."""
    k1, k2, p1, p2, k3 = k
    r2 = x * x + y * y
    radial = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
    return (x * radial + 2 * p1 * x * y + p2 * (r2 + 2 * x * x),
            y * radial + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y)


def undistort_pixels(pts, camera_mtx, dist, iters=5):
    """cv2.undistortPoints(pts, K, dist, P=K): normalise, `iters` fixed-point steps of the inverse model, re-project."""
    K = np.asarray(camera_mtx, np.float64)
    k1, k2, p1, p2, k3 = np.asarray(dist, np.float64)
    pts = np.asarray(pts, np.float64)
    x0, y0 = (pts[..., 0] - K[0, 2]) / K[0, 0], (pts[..., 1] - K[1, 2]) / K[1, 1]
    x, y = x0, y0
    for _ in range(iters):
        r2 = x * x + y * y
        inv = 1.0 / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x, y = (x0 - dx) * inv, (y0 - dy) * inv
    w = K[2, 0] * x + K[2, 1] * y + K[2, 2]
    return np.stack([(K[0, 0] * x + K[0, 1] * y + K[0, 2]) / w, (K[1, 0] * x + K[1, 1] * y + K[1, 2]) / w], -1)


def distort_pixels(pts, camera_mtx, dist):
    K = np.asarray(camera_mtx, np.float64)
    pts = np.asarray(pts, np.float64)
    x, y = (pts[..., 0] - K[0, 2]) / K[0, 0], (pts[..., 1] - K[1, 2]) / K[1, 1]
    xd, yd = distort_normalized(x, y, np.asarray(dist, np.float64))
    return np.stack([K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]], -1)


def undistort_keypoints(kp, camera_mtx, dist, width=1920):
    """dataloader_video.py:441-458: keypoints [...,3] = (x, y, confidence); x is mirrored around the undistortion."""
    kp = np.asarray(kp, np.float64)
    flipped = np.stack([width - 1 - kp[..., 0], kp[..., 1]], -1)
    und = undistort_pixels(flipped, camera_mtx, dist)
    return np.stack([width - 1 - und[..., 0], und[..., 1], kp[..., 2]], -1)


# ---- masks ---------------------------------------------------------------------------------------------------------------
def visibility_masks(kp, mask_joint):
    """dataloader_video.py:462-484.  kp [...,22,3], mask_joint [..., >=22] -> (mask_joint_vis [...,22], mask_vec_vis [...,294])."""
    jv = (np.asarray(kp, np.float64)[..., 2] > 0.2) * np.asarray(mask_joint, np.float64)[..., :22]
    lead = jv.shape[:-1]
    vec = np.ones(lead + (294,))
    off = 0
    for name in G.REPR_LIST:
        d = G.REPR_DIM[name]
        if name in ('local_positions', 'local_vel'):
            vec[..., off:off + d] = np.repeat(jv, 3, axis=-1)
        elif name == 'smplx_body_pose_6d':
            vec[..., off:off + d] = np.repeat(jv[..., 1:], 6, axis=-1)
        elif name == 'foot_contact':
            left = (jv[..., 7] == 1) & (jv[..., 10] == 1)
            right = (jv[..., 8] == 1) & (jv[..., 11] == 1)
            vec[..., off:off + d] = np.stack([left, left, right, right], -1).astype(np.float64)
        off += d
    return jv, vec


def contact_margin(cano_joints):
    """Smallest relative distance of any foot-contact decision of `get_repr_smplx` to its thresholds (velocity 5e-5,
    heights 0.18 / 0.15), over clips [C,T,22,3]."""
    p = np.asarray(cano_joints, np.float64)
    best = np.inf
    for j, h in ((7, 0.18), (10, 0.15), (8, 0.18), (11, 0.15)):
        sq = ((p[:, 1:, j] - p[:, :-1, j]) ** 2).sum(-1)
        best = min(best, np.abs(sq / 5e-5 - 1).min(), np.abs(p[:, :-1, j, 2] / h - 1).min())
    return best


def n_windows(n_frames, clip_len, overlap):
    return len(window_starts(n_frames, clip_len, overlap))


# ---- tolerances of the representation ----------------------------------------------------------------------------------------
def facing_term(cano):
    """[C, T-1]: 3e-6 / |across_xy| + 4e-6 / w of oracle.rederive.facing_margin, frame t taking the worse of frames t, t+1
    (as tests/test_gpu_rederive.py::_close)."""
    raw_xy, w = (np.nan_to_num(v, nan=0.0) for v in RD.facing_margin(np.asarray(cano)))
    pair = lambda v: np.maximum(np.minimum(v[:, :-1], v[:, 1:]), 1e-12)
    return 3e-6 / pair(raw_xy) + 4e-6 / pair(w)


def local_lengths(cano):
    """[C, T-1, 132]: length in metres (at least 1) of the vector behind every local_positions / local_vel channel."""
    p = np.asarray(cano, np.float64)
    lp = p[:, :-1].copy()
    lp[..., :2] -= p[:, :-1, 0:1, :2]
    ln = np.concatenate([np.repeat(np.linalg.norm(lp, axis=-1), 3, axis=-1),
                         np.repeat(np.linalg.norm(p[:, 1:] - p[:, :-1], axis=-1), 3, axis=-1)], axis=-1)
    return np.maximum(np.nan_to_num(ln, nan=0.0), 1.0)


def repr_limits(ref, cano, std, tol, local_factor):
    term = facing_term(cano)
    lim = np.full(np.shape(ref), tol)
    for c in (0, 1, 4, 5):
        lim[:, :, c] = tol + term
    lim[:, :, 22:154] = tol + local_factor * term[:, :, None] * local_lengths(cano)
    return lim


def local_ratio(r32, r64, cano, std=None):
    """Largest |float32 flow - float64 flow| / (term * max(len, 1)) over channels 22..153 (NaN entries skipped)."""
    d = np.abs(np.asarray(r32) - np.asarray(r64))[:, :, 22:154]
    if std is not None:
        d = d / np.asarray(std, np.float64)[22:154]
    with np.errstate(invalid='ignore'):
        return float(np.nanmax(d / (facing_term(cano)[:, :, None] * local_lengths(cano))))
