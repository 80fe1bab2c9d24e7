"""The mask schedules of RoHM's training loops: the decisions on the host, the masking on the device.

`PoseMaskSchedule` restates train/training_loop_posenet.py:107-205 (and :221-248 for the eval block), `TrajMaskSchedule`
train/training_loop_trajnet.py:69-82, `ProxMaskBank` the PROX clips of training_loop_posenet.py:65-98.  A step's decision is a
handful of integers per item; it is drawn from the same global generators (`random`, `torch`, `numpy.random`) with the same calls
in the same order as the reference, so after `random.seed`, `torch.manual_seed` and `np.random.seed` the reference's masks come
out.  The decision goes to the device in one copy and `rohm_train_cond` / `rohm_train_traj_window` (csrc/train_masks.hip) apply
it; there is no CPU fallback.

Stated differences from the reference:
  * the PROX recordings are listed with `sorted(os.listdir(...))`; the reference's unsorted listing depends on the file system;
  * a PROX clip is kept as one uint32 word per frame (bit j: joint j visible) on the device, not as a [clip_len, 294] float64 row
    on the host, and `np.random.shuffle(prox_mask_list)` is reproduced by shuffling a persistent index vector (the same draws,
    the same cumulative order).
"""
from __future__ import annotations

import ctypes as C
import os
import random
from dataclasses import dataclass, field

import numpy as np
import torch

from .._lib import RohmHipError, check, lib, ptr, require_hip, stream_ptr

N_CHANNELS = 294
LOWER_JOINTS = (1, 2, 4, 5, 7, 8, 10, 11)
UPPER_JOINTS = (3, 6, 9, 12, 13, 14, 15, 16, 17, 18, 19, 20)
FULL_MASK_LEN = 30
PROX_MIN_RATIO = 0.05
PROB_DICTS = {
    'lower': {'prox': 0.7, 'lower': 1.0},
    'lower+upper': {'prox': 0.5, 'lower': 0.8, 'upper': 1.0},
    'lower+full': {'prox': 0.5, 'lower': 0.8, 'full': 1.0},
    'lower+upper+full': {'prox': 0.5, 'lower': 0.8, 'upper': 0.9, 'full': 1.0},
}


def joint_bits(joints):
    out = 0
    for j in joints:
        if not 0 <= int(j) < 32:
            raise ValueError(f'joint {j} outside [0, 32)')
        out |= 1 << int(j)
    return out


# ---- the device side ---------------------------------------------------------------------------------------------------------------
def _small(x, dtype, device):
    """A small per-item array for the device: host arrays are uploaded, device tensors pass through."""
    if x is None:
        return None
    if isinstance(x, torch.Tensor):
        if x.dtype != dtype:
            raise ValueError(f'expected {dtype}, got {x.dtype}')
        return x.to(device).contiguous()
    a = np.ascontiguousarray(x)
    if dtype == torch.int32:
        a = a.astype(np.uint32, copy=False).view(np.int32) if a.dtype == np.uint32 else a.astype(np.int32, copy=False)
    else:
        a = a.astype(np.int64, copy=False)
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def train_cond(src, clean=None, joint_bits=None, window=None, vis_bits=None, vis_index=None, zero_contact=False):
    """PoseNet's training condition of a batch in one launch (rohm_train_cond, include/rohm_hip.h).

    src [B, T, 294] float32 on the device -> cond [B, 294, 1, T]; with `clean` [B, T, 294] also its transpose.  Per item, each
    optional: joint_bits [B] (bit j: joint j hidden), window [B, 2] (start, end), vis_bits [n, rows] with vis_index [B] (bit j of
    row f: joint j visible at frame f; multiplied in).  The words are int32 tensors on the device (the bit pattern of the uint32)
    or host arrays, which are uploaded; a host vis_index is range-checked before the launch.  Returns (cond, clean_t or None)."""
    if (vis_bits is None) != (vis_index is None):
        raise ValueError('vis_bits and vis_index go together')
    require_hip(src, clean)
    B, dev = int(src.shape[0]), src.device
    host_index = None
    if vis_index is not None and not (isinstance(vis_index, torch.Tensor) and vis_index.is_cuda):
        host_index = np.ascontiguousarray(vis_index.numpy() if isinstance(vis_index, torch.Tensor) else vis_index, dtype=np.int64)
    jb, win = _small(joint_bits, torch.int32, dev), _small(window, torch.int32, dev)
    vb, vi = _small(vis_bits, torch.int32, dev), _small(vis_index, torch.int64, dev)
    for name, t, shape in (('joint_bits', jb, (B,)), ('window', win, (B, 2)), ('vis_index', vi, (B,))):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f'{name} must have shape {shape}, got {tuple(t.shape)}')
    return _launch_cond(src, clean, jb, win, vb, vi, host_index, zero_contact)


def _launch_cond(src, clean, jb, win, vis_bits, vis_index_dev, vis_index_host, zero_contact):
    """rohm_train_cond on device tensors (or slices of one decision buffer); the host copy of the clip indices, when given, is
    range-checked by the library before the launch."""
    if src.dim() != 3 or src.shape[2] != N_CHANNELS or src.dtype != torch.float32:
        raise ValueError(f'src must be float32 [B,T,{N_CHANNELS}], got {src.dtype} {tuple(src.shape)}')
    if clean is not None and (clean.shape != src.shape or clean.dtype != torch.float32):
        raise ValueError(f'clean must be float32 {tuple(src.shape)}, got {clean.dtype} {tuple(clean.shape)}')
    require_hip(src, clean)
    if vis_bits is not None and vis_bits.dim() != 2:
        raise ValueError('vis_bits must be [n_clips, rows]')
    B, T, dev = int(src.shape[0]), int(src.shape[1]), src.device
    n_vis, vis_rows = (int(vis_bits.shape[0]), int(vis_bits.shape[1])) if vis_bits is not None else (0, 0)
    cond = torch.empty(B, N_CHANNELS, 1, T, device=dev, dtype=torch.float32)
    clean_t = torch.empty_like(cond) if clean is not None else None
    hp = None
    if vis_index_host is not None:
        vis_index_host = np.ascontiguousarray(vis_index_host, dtype=np.int64)
        hp = vis_index_host.ctypes.data_as(C.POINTER(C.c_int64))
    raw = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    with torch.cuda.device(dev):
        check(lib().rohm_train_cond(ptr(src.contiguous()), ptr(clean.contiguous() if clean is not None else None), B, T,
                                    raw(jb), raw(win), ptr(vis_bits), n_vis, vis_rows, raw(vis_index_dev), hp,
                                    int(bool(zero_contact)), ptr(cond), ptr(clean_t), stream_ptr(dev)), 'rohm_train_cond')
    return cond, clean_t


def traj_window(cond, window, n_ch):
    """training_loop_trajnet.py:78-82 in place on cond [B, T, C] (device float32, contiguous): the first n_ch channels of frames
    window[b][0] <= t < window[b][1] are multiplied by 0.  window: [B, 2] int32, on the host or on the device."""
    require_hip(cond)
    if cond.dim() != 3 or cond.dtype != torch.float32 or not cond.is_contiguous():
        raise ValueError(f'cond must be a contiguous float32 [B,T,C] tensor, got {cond.dtype} {tuple(cond.shape)}')
    B, T, Cc = (int(s) for s in cond.shape)
    win = _small(window, torch.int32, cond.device)
    if tuple(win.shape) != (B, 2):
        raise ValueError(f'window must have shape {(B, 2)}, got {tuple(win.shape)}')
    with torch.cuda.device(cond.device):
        check(lib().rohm_train_traj_window(ptr(cond), B, T, Cc, int(n_ch), ptr(win), stream_ptr(cond.device)),
              'rohm_train_traj_window')
    return cond


# ---- PROX mask clips ----------------------------------------------------------------------------------------------------------------
def pack_prox_clips(masks, clip_len, min_ratio=PROX_MIN_RATIO):
    """training_loop_posenet.py:71-96 on a list of mask_joint arrays [N_i, >= 22] (1 = visible): consecutive clips of clip_len
    frames whose hidden-joint ratio over the first 22 joints is at least min_ratio, as uint32 words [n, clip_len] (bit j: joint j
    visible).  The reference multiplies by the mask values themselves, so values other than 0 and 1 are refused."""
    words = []
    shifts = np.arange(22, dtype=np.uint32)[None]
    for mask in masks:
        mask = np.asarray(mask)
        for i in range(len(mask) // clip_len):
            clip = mask[i * clip_len:(i + 1) * clip_len][:, 0:22]
            if not np.isin(clip, (0, 1)).all():
                raise ValueError('PROX joint masks must hold only 0 and 1')
            all_joints_n = clip.shape[0] * clip.shape[1]
            mask_ratio = (all_joints_n - clip.sum()) / all_joints_n
            if mask_ratio >= min_ratio:
                words.append((clip.astype(np.uint32) << shifts).sum(axis=1).astype(np.uint32))
    return np.asarray(words, dtype=np.uint32).reshape(len(words), clip_len)


class ProxMaskBank:
    """The PROX joint-mask clips of the loop, 4 bytes per frame on the device.

    `root` is the directory that holds `PROX/mask_joint/<recording>/mask_joint.npy` (the parent of the drivers' dataset_root);
    `masks` gives the arrays directly instead.  `draw(bs)` is `np.random.shuffle(prox_mask_list); prox_mask_list[0:bs]` as clip
    indices: the persistent order vector takes the same draws as the reference's array and ends in the same order."""

    def __init__(self, root=None, clip_len=145, device='cuda', masks=None):
        if masks is None:
            base = os.path.join(root, 'PROX', 'mask_joint')
            self.recordings = sorted(os.listdir(base))
            masks = [np.load(os.path.join(base, d, 'mask_joint.npy')) for d in self.recordings]
        self.clip_len = int(clip_len)
        self.bits_host = pack_prox_clips(masks, self.clip_len)
        self.order = np.arange(len(self.bits_host), dtype=np.int64)
        self.device = torch.device(device)
        self._bits = None

    def __len__(self):
        return len(self.bits_host)

    @property
    def bits(self):
        """[n, clip_len] int32 on the device (the uint32 words' bit patterns)."""
        if self._bits is None:
            if self.device.type != 'cuda':
                raise RohmHipError('the PROX masks are applied on an AMD GPU; there is no CPU fallback')
            self._bits = torch.from_numpy(self.bits_host.view(np.int32)).to(self.device)
        return self._bits

    def draw(self, bs):
        if len(self) < bs:
            raise ValueError(f'{len(self)} PROX mask clips cannot fill a batch of {bs}')
        np.random.shuffle(self.order)
        return self.order[:bs].copy()


# ---- the schedules -------------------------------------------------------------------------------------------------------------------
@dataclass
class PoseMaskDecision:
    """What one step hides.  branch: 'joints' (1-6 random joints per item), 'prox', 'lower', 'upper', 'full' or 'none'."""
    branch: str
    joint_bits: np.ndarray | None = None       # [B] uint32
    window: np.ndarray | None = None           # [B, 2] int32
    vis_index: np.ndarray | None = None        # [B] int64 clips of the bank
    zero_contact: bool = False
    joints: list = field(default_factory=list)  # the drawn joint ids (per item for 'joints', one set otherwise)


class PoseMaskSchedule:
    """training_loop_posenet.py:107-205: up to and including epoch start_prox_mask_epoch 1-6 random joints per item are hidden;
    afterwards one of the PROX clips / the lower body / the upper body (5 of its joints plus both arms' ends, or all) / a
    30-frame window of the whole body, by mask_scheme's probabilities.  With input_noise the contact channels are always hidden
    and the condition is made from the noisy rows."""

    def __init__(self, start_prox_mask_epoch, mask_scheme, input_noise, prox_bank=None):
        if mask_scheme not in PROB_DICTS:
            raise ValueError(f'mask_scheme must be one of {sorted(PROB_DICTS)}, got {mask_scheme!r}')
        self.start_prox_mask_epoch, self.mask_scheme, self.input_noise = start_prox_mask_epoch, mask_scheme, bool(input_noise)
        self.prox_bank = prox_bank

    # -- host decisions ----------------------------------------------------------------------------------------------------------
    def _random_joints(self, bs):
        mask_joint_n = random.randint(1, 6)
        mask_joint_id = (torch.rand(bs, mask_joint_n) * 22).long()
        mask_joint_id[mask_joint_id == 0] = 1      # never the pelvis
        ids = mask_joint_id.numpy()
        bits = np.asarray([joint_bits(row) for row in ids], dtype=np.uint32).reshape(bs)
        return PoseMaskDecision('joints', joint_bits=bits, zero_contact=self.input_noise, joints=ids.tolist())

    def decide_eval(self, bs):
        """The eval block's masks (:227-245): always the random joints."""
        return self._random_joints(bs)

    def decide(self, epoch, bs, T):
        """The decision of a training step on a batch of bs items of T frames."""
        if epoch <= self.start_prox_mask_epoch:
            return self._random_joints(bs)
        prob = random.uniform(0, 1)
        prob_dict = PROB_DICTS[self.mask_scheme]
        if prob <= prob_dict['prox']:
            if self.prox_bank is None:
                raise ValueError('the PROX branch of the mask schedule needs a ProxMaskBank')
            if self.prox_bank.clip_len < T:
                raise ValueError(f'PROX clips of {self.prox_bank.clip_len} frames cannot mask {T} frames')
            return PoseMaskDecision('prox', vis_index=self.prox_bank.draw(bs), zero_contact=self.input_noise)
        if prob <= prob_dict['lower']:
            bits = np.full(bs, joint_bits(LOWER_JOINTS), dtype=np.uint32)
            return PoseMaskDecision('lower', joint_bits=bits, zero_contact=True, joints=list(LOWER_JOINTS))
        if 'upper' in prob_dict and prob <= prob_dict['upper']:
            if random.uniform(0, 1) < 0.6:
                select = random.sample(list(UPPER_JOINTS), 5)
                select = sorted(select + [j for j in (18, 19, 20, 21) if j not in select])
            else:
                select = list(UPPER_JOINTS)
            bits = np.full(bs, joint_bits(select), dtype=np.uint32)
            return PoseMaskDecision('upper', joint_bits=bits, zero_contact=True, joints=select)
        if 'full' in prob_dict and prob <= prob_dict['full']:
            start = torch.FloatTensor(bs).uniform_(0, T - 1).long()
            end = start + FULL_MASK_LEN
            end[end > T] = T
            window = torch.stack([start, end], dim=1).numpy().astype(np.int32)
            return PoseMaskDecision('full', window=window, zero_contact=True)
        return PoseMaskDecision('none', zero_contact=self.input_noise)

    # -- device ------------------------------------------------------------------------------------------------------------------
    def apply(self, decision, src, clean=None):
        """(cond [B, 294, 1, T], clean_t or None): the decision's arrays go to the device in one copy."""
        B, dev = int(src.shape[0]), src.device
        d = decision
        # one int32 buffer: [vis_index as int64: 2B | joint_bits: B | window: 2B]
        buf = np.zeros(5 * B, dtype=np.int32)
        if d.vis_index is not None:
            buf[:2 * B].view(np.int64)[:] = d.vis_index
        if d.joint_bits is not None:
            buf[2 * B:3 * B].view(np.uint32)[:] = d.joint_bits
        if d.window is not None:
            buf[3 * B:].reshape(B, 2)[:] = d.window
        require_hip(src)
        dbuf = torch.from_numpy(buf).to(dev, non_blocking=True)
        vis_bits = self.prox_bank.bits if d.vis_index is not None else None
        cond, clean_t = _launch_cond(src, clean, dbuf[2 * B:3 * B] if d.joint_bits is not None else None,
                                            dbuf[3 * B:].view(B, 2) if d.window is not None else None, vis_bits,
                                            dbuf[:2 * B].view(torch.int64) if d.vis_index is not None else None, d.vis_index,
                                            d.zero_contact)
        return cond, clean_t

    def __call__(self, batch, epoch, eval_block=False):
        """The loop's mask block on a device batch, in place: batch['cond'] and batch['motion_repr_clean'] become
        [B, 294, 1, T].  Returns the decision."""
        clean = batch['motion_repr_clean']
        src = batch['motion_repr_noisy'] if self.input_noise else clean
        B, T = int(clean.shape[0]), int(clean.shape[1])
        decision = self.decide_eval(B) if eval_block else self.decide(epoch, B, T)
        batch['cond'], batch['motion_repr_clean'] = self.apply(decision, src, clean)
        return decision


@dataclass
class TrajMaskDecision:
    window: np.ndarray | None = None           # [B, 2] int32, None: no mask this step


class TrajMaskSchedule:
    """training_loop_trajnet.py:69-82: from epoch start_infill_epoch on, with probability mask_prob, a window of up to
    max_infill_ratio of the clip loses the trajectory channels of batch['cond']."""

    def __init__(self, start_infill_epoch, mask_prob, max_infill_ratio):
        self.start_infill_epoch, self.mask_prob, self.max_infill_ratio = start_infill_epoch, mask_prob, max_infill_ratio

    def decide(self, epoch, bs, T):
        if epoch < self.start_infill_epoch:
            return TrajMaskDecision()
        prob = random.uniform(0, 1)
        if not prob > 1 - self.mask_prob:
            return TrajMaskDecision()
        start = torch.FloatTensor(bs).uniform_(0, T - 1).long()
        mask_len = (T * torch.FloatTensor(bs).uniform_(0, 1) * self.max_infill_ratio).long()
        end = start + mask_len
        end[end > T] = T
        return TrajMaskDecision(torch.stack([start, end], dim=1).numpy().astype(np.int32))

    def __call__(self, batch, epoch, traj_feat_dim):
        """The loop's mask block on a device batch: batch['cond'] [B, T, C] is masked in place.  Returns the decision."""
        cond = batch['cond']
        decision = self.decide(epoch, int(cond.shape[0]), int(cond.shape[1]))
        if decision.window is not None:
            if not cond.is_contiguous():
                cond = batch['cond'] = cond.contiguous()
            traj_window(cond, decision.window, traj_feat_dim)
        return decision
