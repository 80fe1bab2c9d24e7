"""A numpy restatement of the training loops' condition masks (test infrastructure; CPU only).

The rules are those of the reference's loops: the per-joint zeroing of training_loop_posenet.py:120-132 (and :232-245), the PROX
visibility vector of :80-95, the window of :194-200 and the trajectory window of training_loop_trajnet.py:74-82, stated over
whole arrays instead of per-item assignments.  Nothing here calls the package under test."""
import numpy as np

C, TRAJ = 294, 22
POS0, VEL0, POSE0, BETAS0, CONTACT0 = 22, 88, 154, 280, 290
LOWER = (1, 2, 4, 5, 7, 8, 10, 11)
UPPER = (3, 6, 9, 12, 13, 14, 15, 16, 17, 18, 19, 20)


def joint_channels(j):
    """The channels the loops zero for joint j (contacts excluded)."""
    ch = [POS0 + 3 * j + k for k in range(3)] + [VEL0 + 3 * j + k for k in range(3)]
    if j >= 1:
        ch += [POSE0 + 6 * (j - 1) + k for k in range(6)]
    return ch


def bits_of(joints):
    out = 0
    for j in joints:
        out |= 1 << int(j)
    return out


def joints_of(bits):
    return [j for j in range(32) if (int(bits) >> j) & 1]


def vis_vector(bits_rows):
    """[T] visibility words (bit j: joint j visible) -> the 0 / 1 float64 vector [T, 294] of :80-95."""
    bits_rows = np.asarray(bits_rows, dtype=np.uint32)
    T = bits_rows.shape[0]
    vis = ((bits_rows[:, None] >> np.arange(22, dtype=np.uint32)[None]) & 1).astype(np.float64)      # [T, 22]
    out = np.ones((T, C))
    out[:, POS0:VEL0] = vis.repeat(3, axis=1)
    out[:, VEL0:POSE0] = vis.repeat(3, axis=1)
    out[:, POSE0:BETAS0] = vis[:, 1:].repeat(6, axis=1)
    out[:, CONTACT0:] = 0.0
    out[(vis[:, 7] == 1) & (vis[:, 10] == 1), CONTACT0:CONTACT0 + 2] = 1.0
    out[(vis[:, 8] == 1) & (vis[:, 11] == 1), CONTACT0 + 2:] = 1.0
    return out


def train_cond(src, joint_bits=None, window=None, vis_bits=None, vis_index=None, zero_contact=False):
    """src [B, T, 294] float32 -> cond [B, 294, 1, T] float32: the multiplication by the visibility vector first, then the
    assignments of 0."""
    src = np.asarray(src, dtype=np.float32)
    B, T, _ = src.shape
    cond = src.copy()
    for b in range(B):
        if vis_bits is not None:
            cond[b] = cond[b] * vis_vector(np.asarray(vis_bits)[int(vis_index[b]), :T]).astype(np.float32)
        if joint_bits is not None:
            js = joints_of(joint_bits[b])
            for j in js:
                cond[b][:, joint_channels(j)] = 0.0
            if 7 in js or 10 in js:
                cond[b][:, CONTACT0:CONTACT0 + 2] = 0.0
            if 8 in js or 11 in js:
                cond[b][:, CONTACT0 + 2:] = 0.0
        if window is not None:
            s, e = int(window[b][0]), int(window[b][1])
            if e > s:
                cond[b][max(s, 0):e, TRAJ:] = 0.0
    if zero_contact:
        cond[:, :, CONTACT0:] = 0.0
    return np.ascontiguousarray(cond.transpose(0, 2, 1)[:, :, None, :])


def transpose(x):
    return np.ascontiguousarray(np.asarray(x).transpose(0, 2, 1)[:, :, None, :])


def traj_window(cond, window, n_ch):
    """cond [B, T, C] -> a copy with the first n_ch channels multiplied by 0 inside [start, end) and by 1 outside."""
    out = np.array(cond, dtype=np.float32, copy=True)
    B, T, _ = out.shape
    m = np.ones((B, T), dtype=np.float32)
    for b in range(B):
        s, e = int(window[b][0]), int(window[b][1])
        if e > s:
            m[b, max(s, 0):e] = 0.0
    out[:, :, :n_ch] = out[:, :, :n_ch] * m[:, :, None]
    return out


def pack_visibility(mask_clip):
    """[T, >= 22] 0 / 1 visibility -> [T] uint32 words."""
    m = np.asarray(mask_clip)[:, :22]
    return (m.astype(np.uint32) << np.arange(22, dtype=np.uint32)[None]).sum(axis=1).astype(np.uint32)
