"""Native AMASS loader: the reference's `data_loaders/dataloader_amass.py` with its per-clip work on the device.

The host part only reads the pre-processed sequences (`divide_clip`) and, without `load_noise`, draws the parameter
noise with `np.random.normal` in the reference's order, so that a run after `np.random.seed(k)` builds the reference's
dataset.  Everything else is launches over chunks of clips: `clips.build_clips` (canonicalise + clean representation),
`param_noise` (Euler-space SMPL-X noise, float64), `frames.noisy_clip_joints` (FK of the noisy parameters),
`clips.clips_repr` (noisy representation), `repr_stats` (dataset statistics, split 'train') and `assemble` (the
normalised items of `__getitem__`).

`__len__` / `__getitem__` return the reference's items as host numpy (same keys, shapes and dtypes), made from one
device -> host copy at construction, so the object works in a `torch.utils.data.DataLoader` with workers without touching
the GPU there.  `batches(batch_size, shuffle, drop_last, generator)` yields the collated dicts as device tensors, one
`rohm_amass_batch` launch per batch; its rows equal the `__getitem__` rows bit for bit.

With `sep_noise=True` an item's noise is drawn when the item is made, as in the reference: `__getitem__` draws with
`np.random.normal` in the reference's order and needs the device; `batches()` draws on the device from `generator`.

Kept quirks of the reference: `ceil(n_samples / spacing)` clips are built but `__len__` is `n_samples // spacing`, and
with `load_noise` clip i (which already steps by `spacing`) takes row `i * spacing` of the loaded noise."""
from __future__ import annotations

import glob
import os
import pickle

import numpy as np
import torch
from torch.utils import data

from .. import _lib
from .._lib import check, lib, ptr, require_hip, stream_ptr
from . import clips, frames
from .dataloader_video import ABS_TRAJ_CH, REPR_DIM_DICT, REPR_LIST, _body_model, read_stats

NOISE_ORDER = ('transl', 'body_pose', 'betas', 'global_orient')          # the draw order per clip (:159)
SEP_NOISE_ORDER = ('global_orient', 'transl', 'body_pose', 'betas')      # the draw order per sep_noise item (:300)
PARAM_COLS = {'global_orient': (0, 3), 'transl': (3, 6), 'betas': (6, 16), 'body_pose': (16, 79)}


# ---- host reader ------------------------------------------------------------------------------------------------------
def read_amass_clips(root, amass_datasets, split, clip_len):
    """`divide_clip` for every dataset: (joints [F,22,3] float32, smplx [F,79] float64, starts [n] int32) -- the frames
    of all kept clips back to back and the first frame of every clip."""
    joints, smplx, starts, at = [], [], [], 0
    for name in amass_datasets:
        for path in sorted(glob.glob(os.path.join(root, 'pose_data_fps_30', name, '*/*.npy'))):
            seq, npy = path.split('/')[-2:]
            j = np.load(path)
            s = np.load(os.path.join(root, 'smpl_data_fps_30', name, seq, npy))
            if split == 'test':
                j, s = j[1:-1], s[1:-1]
            if len(j) < clip_len:
                continue
            keep = int(len(j) / clip_len) * clip_len
            joints.append(np.asarray(j[:keep, 0:22], dtype=np.float32))
            smplx.append(np.asarray(s[:keep, 0:79], dtype=np.float64))
            starts.extend(range(at, at + keep, clip_len))
            at += keep
    if not joints:
        return np.zeros((0, 22, 3), np.float32), np.zeros((0, 79)), np.zeros(0, np.int32)
    return np.concatenate(joints), np.concatenate(smplx), np.asarray(starts, dtype=np.int32)


# ---- device operators ------------------------------------------------------------------------------------------------------
def _f64(x, shape, name, device):
    if not torch.is_tensor(x) or x.dtype != torch.float64 or tuple(x.shape) != shape or x.device != device:
        raise ValueError(f'{name} must be a float64 tensor {shape} on {device}')
    return x.contiguous()


def param_noise(params, noise, additive=False):
    """SMPL-X parameter noise (dataloader_amass.py:156-192) on params [..., 79] (device float64 rows global_orient,
    transl, betas, body_pose).  noise: dict of device float64 tensors 'global_orient' [...,3] and 'body_pose' [...,63] or
    [...,21,3] (degrees, added to the 'zxy' Euler angles), 'transl' [...,3], 'betas' [...,10].  additive=True adds all
    four to the parameters as they are (the sep_noise items).  Returns the noisy parameters, same shape."""
    require_hip(params, *noise.values())
    if params.dim() < 2 or params.shape[-1] != 79 or params.dtype != torch.float64:
        raise ValueError(f'params must be float64 [...,79], got {params.dtype} {tuple(params.shape)}')
    lead, dev = tuple(params.shape[:-1]), params.device
    M = int(np.prod(lead))
    bp = noise['body_pose']
    if torch.is_tensor(bp) and tuple(bp.shape) == lead + (21, 3):
        bp = bp.reshape(lead + (63,))
    nz = {'global_orient': _f64(noise['global_orient'], lead + (3,), "noise['global_orient']", dev),
          'transl': _f64(noise['transl'], lead + (3,), "noise['transl']", dev),
          'betas': _f64(noise['betas'], lead + (10,), "noise['betas']", dev),
          'body_pose': _f64(bp, lead + (63,), "noise['body_pose']", dev)}
    out = torch.empty_like(params, memory_format=torch.contiguous_format)
    with torch.cuda.device(dev):
        check(lib().rohm_smplx_param_noise(ptr(params.contiguous()), ptr(nz['global_orient']), ptr(nz['transl']), ptr(nz['betas']),
                                           ptr(nz['body_pose']), M, int(bool(additive)), ptr(out), stream_ptr(dev)),
              'rohm_smplx_param_noise')
    return out


def repr_stats(repr_clean):
    """Per-channel mean and population std of a de-normalised representation [..., 294] (device float32), accumulated in
    float64 in a fixed order -> (mean [294], std [294]) device float64."""
    require_hip(repr_clean)
    if repr_clean.dim() < 2 or repr_clean.shape[-1] != 294 or repr_clean.dtype != torch.float32:
        raise ValueError(f'repr must be float32 [...,294], got {repr_clean.dtype} {tuple(repr_clean.shape)}')
    rows = repr_clean.numel() // 294
    if rows < 1:
        raise ValueError('repr_stats needs at least one row')
    dev = repr_clean.device
    mean, std = (torch.empty(294, device=dev, dtype=torch.float64) for _ in range(2))
    nbytes = lib().rohm_repr_stats_scratch_bytes(rows)
    scratch = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        check(lib().rohm_repr_stats(ptr(repr_clean.contiguous()), rows, ptr(mean), ptr(std), ptr(scratch), nbytes, stream_ptr(dev)),
              'rohm_repr_stats')
    return mean, std


def assemble(repr_clean, repr_noisy, index, mean, std, overwrite_channels=0, cond=None, control=False, noisy_per_batch=False):
    """dataloader_amass.py:317-339 for the items `index` (device int64 [B]): repr_clean / repr_noisy [n, R, 294]
    de-normalised float32 (repr_noisy None: the noisy item is the clean one; with noisy_per_batch it is [B, R, 294]),
    mean / std [294] float32.  overwrite_channels: the leading noisy channels taken from the clean item (task 'pose').
    cond: None, 'traj' (first 22 channels) or 'abs' (the 13 absolute ones); control: also the last 272 clean channels.
    Returns a dict of float32 tensors 'motion_repr_clean', 'motion_repr_noisy' [B, R, 294] (+ 'cond', 'control_cond')."""
    require_hip(repr_clean, repr_noisy, index, mean, std)
    if repr_clean.dim() != 3 or repr_clean.shape[2] != 294 or repr_clean.dtype != torch.float32:
        raise ValueError(f'repr_clean must be float32 [n,R,294], got {repr_clean.dtype} {tuple(repr_clean.shape)}')
    n, R = int(repr_clean.shape[0]), int(repr_clean.shape[1])
    if index.dim() != 1 or index.dtype != torch.int64:
        raise ValueError('index must be a 1-D int64 tensor')
    B, dev = int(index.shape[0]), repr_clean.device
    if repr_noisy is not None and (repr_noisy.dtype != torch.float32 or
                                   tuple(repr_noisy.shape) != ((B if noisy_per_batch else n), R, 294)):
        raise ValueError(f'repr_noisy must be float32 [{B if noisy_per_batch else n},{R},294], got {tuple(repr_noisy.shape)}')
    if cond not in (None, 'traj', 'abs'):
        raise ValueError(f"cond must be None, 'traj' or 'abs', got {cond!r}")
    if not 0 <= int(overwrite_channels) <= 294:
        raise ValueError('overwrite_channels must be in [0, 294]')
    if mean.shape != (294,) or std.shape != (294,) or mean.dtype != torch.float32 or std.dtype != torch.float32:
        raise ValueError('mean and std must be float32 [294]')
    if R < 1:
        raise ValueError('items need at least one row')
    f32 = dict(device=dev, dtype=torch.float32)
    out = {'motion_repr_clean': torch.empty(B, R, 294, **f32), 'motion_repr_noisy': torch.empty(B, R, 294, **f32)}
    if cond:
        out['cond'] = torch.empty(B, R, 22 if cond == 'traj' else 13, **f32)
    if control:
        out['control_cond'] = torch.empty(B, R, 272, **f32)
    if B:
        with torch.cuda.device(dev):
            check(lib().rohm_amass_batch(ptr(repr_clean.contiguous()), ptr(repr_noisy.contiguous() if repr_noisy is not None else None),
                                         n, R, ptr(index.contiguous()), B, ptr(mean.contiguous()), ptr(std.contiguous()),
                                         int(overwrite_channels), int(bool(noisy_per_batch)), {None: 0, 'traj': 1, 'abs': 2}[cond],
                                         ptr(out['motion_repr_clean']), ptr(out['motion_repr_noisy']), ptr(out.get('cond')),
                                         ptr(out.get('control_cond')), stream_ptr(dev)), 'rohm_amass_batch')
    return out


def group_stats(mean64, std64):
    """dataloader_amass.py:255-263 on per-channel float64 mean / std [294]: float32 casts, one std per group (its mean)
    except for smplx_betas, foot_contact mean 0 / std 1 -> (Mean_dict, Std_dict) in REPR_LIST order."""
    mean_dict, std_dict, o = {}, {}, 0
    for name in REPR_LIST:
        d = REPR_DIM_DICT[name]
        m, s = np.asarray(mean64[o:o + d]).astype(np.float32), np.asarray(std64[o:o + d]).astype(np.float32)
        if name == 'foot_contact':
            m[...] = 0.0
            s[...] = 1.0
        elif name != 'smplx_betas':
            s[...] = s.mean() / 1.0
        mean_dict[name], std_dict[name] = m, s
        o += d
    return mean_dict, std_dict


# ---- the dataset --------------------------------------------------------------------------------------------------------------
class DataloaderAMASS(data.Dataset):
    def __init__(self, preprocessed_amass_root='', body_model_path='', amass_datasets=None, split='train', spacing=1,
                 repr_abs_only=False, input_noise=False, sep_noise=False, noise_std_joint=0.0, noise_std_smplx_global_rot=0.0,
                 noise_std_smplx_body_rot=0.0, noise_std_smplx_trans=0.0, noise_std_smplx_betas=0.0, load_noise=False,
                 loaded_smplx_noise_dict=None, task='traj', clip_len=150, joints_num=22, logdir=None, device='cuda',
                 chunk_clips=512):
        if task not in ('traj', 'pose'):
            raise ValueError("task should be in ['traj', 'pose']")
        if split not in ('train', 'test'):
            raise ValueError("split should be in ['train', 'test']")
        if joints_num != 22:
            raise ValueError('the motion representation is defined for joints_num = 22')
        if not isinstance(spacing, (int, np.integer)) or spacing < 1:
            raise ValueError(f'spacing must be a positive integer, got {spacing!r}')
        if not isinstance(chunk_clips, (int, np.integer)) or chunk_clips < 1:
            raise ValueError(f'chunk_clips must be a positive integer, got {chunk_clips!r}')
        clips._check_clip_len(clip_len)
        self.preprocessed_amass_root, self.split, self.clip_len, self.logdir = preprocessed_amass_root, split, clip_len, logdir
        self.spacing, self.joints_num, self.task = spacing, joints_num, task
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise _lib.RohmHipError('DataloaderAMASS builds its clips on an AMD GPU; there is no CPU fallback')
        self.head_joint_idx, self.torso_joint_idx = [15], [12, 9, 6, 3]
        self.input_noise, self.sep_noise, self.noise_std_joint = input_noise, sep_noise, noise_std_joint
        self.noise_std_params_dict = {'global_orient': noise_std_smplx_global_rot, 'transl': noise_std_smplx_trans,
                                      'body_pose': noise_std_smplx_body_rot, 'betas': noise_std_smplx_betas}
        self.load_noise, self.loaded_smplx_noise_dict = load_noise, loaded_smplx_noise_dict
        if input_noise and not sep_noise and load_noise and loaded_smplx_noise_dict is None:
            raise ValueError('load_noise needs loaded_smplx_noise_dict')
        self.repr_abs_only = repr_abs_only
        if not repr_abs_only:
            self.traj_repr_name_list = ['root_rot_angle', 'root_rot_angle_vel', 'root_l_pos', 'root_l_vel', 'root_height',
                                        'smplx_rot_6d', 'smplx_rot_vel', 'smplx_trans', 'smplx_trans_vel']
        else:
            self.traj_repr_name_list = ['root_rot_angle', 'root_l_pos', 'root_height', 'smplx_rot_6d', 'smplx_trans']
        self.local_repr_name_list = ['local_positions', 'local_vel', 'smplx_body_pose_6d', 'smplx_betas', 'foot_contact']
        self.body_feat_dim = sum(REPR_DIM_DICT.values())
        self.traj_feat_dim = sum(REPR_DIM_DICT[k] for k in self.traj_repr_name_list)
        self.pose_feat_dim = sum(REPR_DIM_DICT[k] for k in self.local_repr_name_list)
        self._chunk = int(chunk_clips)
        needs_model = input_noise and not sep_noise
        self.smplx_neutral = _body_model(body_model_path, 'neutral', self.device) if needs_model or \
            isinstance(body_model_path, torch.nn.Module) or body_model_path else None

        joints, smplx, starts = read_amass_clips(preprocessed_amass_root, amass_datasets or [], split, clip_len)
        self.n_samples = int(len(starts))
        print('[INFO] {} set: get {} sub clips in total.'.format(split, self.n_samples))
        self._build(joints, smplx, starts)

    # -- construction ----------------------------------------------------------------------------------------------------
    def _clip_noise(self, k):
        """Host noise of built clip k (source clip i = k * spacing): loaded rows or fresh draws in the reference's order."""
        L, i = self.clip_len, k * self.spacing
        shapes = {'transl': (L, 3), 'body_pose': (L * 21, 3), 'betas': (L, 10), 'global_orient': (L, 3)}
        out = {}
        for name in NOISE_ORDER:
            if self.load_noise:
                out[name] = np.asarray(self.loaded_smplx_noise_dict[name][i * self.spacing], dtype=np.float64)
            else:
                out[name] = np.random.normal(loc=0.0, scale=self.noise_std_params_dict[name], size=shapes[name])
            out[name] = out[name].reshape(L, -1)
            if out[name].shape != (L, PARAM_COLS[name][1] - PARAM_COLS[name][0]):
                raise ValueError(f'noise of {name} for clip {i} has shape {out[name].shape}')
        return out

    def _build(self, joints, smplx, starts):
        dev, L = self.device, self.clip_len
        sel = starts[::self.spacing]
        n = self._n_built = int(len(sel))
        J, W = torch.from_numpy(joints).to(dev), torch.from_numpy(smplx).to(dev)
        with_noise = self.input_noise and not self.sep_noise
        clean, cj, noisy, nj, prm = [], [], [], [], []
        noise_host = {k: [] for k in NOISE_ORDER}
        ar = torch.arange(L, device=dev)
        for a in range(0, n, self._chunk):
            st = torch.from_numpy(np.ascontiguousarray(sel[a:a + self._chunk])).to(dev)
            built = clips.build_clips(J, W, L, 0, up_axis='z', starts=st, params_f64=True)
            c = int(st.shape[0])
            clean.append(built['repr'])
            cj.append(built['cano_joints'])
            if not (with_noise or (self.input_noise and self.sep_noise)):
                continue
            rows = W[st.long()[:, None] + ar[None]]                                                  # [c, L, 79]
            params = torch.cat([built['orient_transl64'], rows[..., 6:79]], dim=-1)
            if not with_noise:
                prm.append(params)
                continue
            per_clip = [self._clip_noise(a + k) for k in range(c)]
            nz = {k: torch.from_numpy(np.stack([p[k] for p in per_clip])).to(dev) for k in NOISE_ORDER}
            for k in NOISE_ORDER:
                noise_host[k].extend(p[k] for p in per_clip)
            noisy_params = param_noise(params, nz)
            flat = noisy_params.reshape(c * L, 79)
            fk = frames.noisy_clip_joints(self.smplx_neutral, {k: flat[:, s:e] for k, (s, e) in PARAM_COLS.items()}, dev)
            fk = fk.reshape(c, L, 22, 3)
            nj.append(fk)
            noisy.append(clips.clips_repr(fk, noisy_params))
        f32 = dict(device=dev, dtype=torch.float32)
        cat = lambda parts, tail, **kw: torch.cat(parts) if parts else torch.empty((0,) + tail, **kw)
        d = {'clean': cat(clean, (L - 1, 294), **f32), 'joints_clean': cat(cj, (L, 22, 3), **f32)}
        if with_noise:
            d['noisy'], d['joints_noisy'] = cat(noisy, (L - 1, 294), **f32), cat(nj, (L, 22, 3), **f32)
            # what the reference would pickle as its noise file: [n, L, 3 | 21, 3 | 10]
            self.smplx_noise_dict = {k: np.asarray(v).reshape((n, L, 21, 3) if k == 'body_pose' else (n, L, -1))
                                     for k, v in noise_host.items()}
        elif self.input_noise:
            d['params'] = cat(prm, (L, 79), device=dev, dtype=torch.float64)

        # ---- statistics
        if self.split == 'train':
            if n == 0:
                raise ValueError('no clip to take the statistics from')
            mean64, std64 = (t.cpu().numpy() for t in repr_stats(d['clean']))
            self.Mean_dict, self.Std_dict = group_stats(mean64, std64)
            os.makedirs(self.logdir, exist_ok=True)
            for fname, dd in (('AMASS_mean.pkl', self.Mean_dict), ('AMASS_std.pkl', self.Std_dict)):
                with open(os.path.join(self.logdir, fname), 'wb') as f:
                    pickle.dump(dd, f, protocol=2)
            self.Mean = np.concatenate([self.Mean_dict[k] for k in self.Mean_dict], axis=-1)
            self.Std = np.concatenate([self.Std_dict[k] for k in self.Std_dict], axis=-1)
        else:
            self.Mean_dict, self.Std_dict, self.Mean, self.Std = read_stats(self.logdir)
        d['mean'] = torch.from_numpy(np.ascontiguousarray(self.Mean, dtype=np.float32)).to(dev)
        d['std'] = torch.from_numpy(np.ascontiguousarray(self.Std, dtype=np.float32)).to(dev)
        self._device_data = d

        # ---- host items: assembled on the device, one device -> host copy
        self._host = {}
        if self.input_noise and self.sep_noise:
            return
        parts = [self._assemble(torch.arange(a, min(a + self._chunk, n), device=dev)) for a in range(0, n, self._chunk)]
        keys = ['motion_repr_clean', 'motion_repr_noisy'] + (['noisy_joints'] if with_noise else [])
        tens = {k: (torch.cat([p[k] for p in parts]) if parts else torch.empty(0, **f32)) for k in keys}
        flat = torch.cat([v.reshape(-1) for v in tens.values()]).cpu().numpy()
        off = 0
        for k, v in tens.items():
            self._host[k] = flat[off:off + v.numel()].reshape(tuple(v.shape))
            off += v.numel()

    def _assemble(self, index, noisy=None, noisy_joints=None):
        """The device batch of items `index`; `noisy` / `noisy_joints` are the per-batch sep_noise rows."""
        d = self._device_data
        per_batch = noisy is not None
        if not per_batch and self.input_noise:
            noisy = d['noisy']
        cond = None if self.task != 'traj' else ('abs' if self.repr_abs_only else 'traj')
        over = self.traj_feat_dim if (self.task == 'pose' and self.input_noise) else 0
        out = assemble(d['clean'], noisy, index, d['mean'], d['std'], over, cond, self.task == 'traj', per_batch)
        batch = {'motion_repr_clean': out['motion_repr_clean']}
        if self.input_noise:
            batch['noisy_joints'] = noisy_joints if per_batch else d['joints_noisy'][index]
        batch['motion_repr_noisy'] = out['motion_repr_noisy']
        if self.task == 'traj':
            batch['cond'], batch['control_cond'] = out['cond'], out['control_cond']
        return batch

    def _sep_noise_rows(self, index, noise):
        """clips_repr of the items `index` with the additive noise `noise` (device float64: the four parameter groups and
        'joints') -> (noisy representation [B, L-1, 294], noisy joints [B, L, 22, 3])."""
        d = self._device_data
        noisy_params = param_noise(d['params'][index], noise, additive=True)
        return clips.clips_repr(d['joints_clean'][index], noisy_params, joint_noise=noise['joints'], return_joints=True)

    # -- the Dataset interface -------------------------------------------------------------------------------------------------
    def __getstate__(self):
        # what a DataLoader worker gets: the host items only, nothing that lives on the device
        return {k: v for k, v in self.__dict__.items() if k not in ('_device_data', 'smplx_neutral')}

    def __len__(self):
        return self.n_samples // self.spacing

    def __getitem__(self, index):
        if self.input_noise and self.sep_noise:
            return self._sep_noise_item(index)
        h = self._host
        item = {'motion_repr_clean': h['motion_repr_clean'][index]}
        if self.input_noise:
            item['noisy_joints'] = h['noisy_joints'][index]
        item['motion_repr_noisy'] = h['motion_repr_noisy'][index]
        if self.task == 'traj':
            t = item['motion_repr_noisy']
            item['cond'] = t[:, list(ABS_TRAJ_CH)] if self.repr_abs_only else t[:, 0:self.traj_feat_dim]
            item['control_cond'] = item['motion_repr_clean'][:, -self.pose_feat_dim:]
        return item

    def _sep_noise_item(self, index):
        if '_device_data' not in self.__dict__:
            raise _lib.RohmHipError('sep_noise items are made on the device: use num_workers=0 or batches()')
        index = int(index)
        if not -self._n_built <= index < self._n_built:
            raise IndexError(index)
        index %= self._n_built
        L, dev = self.clip_len, self.device
        shapes = {'global_orient': (L, 3), 'transl': (L, 3), 'body_pose': (L, 63), 'betas': (L, 10)}
        host = {k: np.random.normal(loc=0.0, scale=self.noise_std_params_dict[k], size=shapes[k]) for k in SEP_NOISE_ORDER}
        host['joints'] = np.random.normal(loc=0.0, scale=self.noise_std_joint, size=(L, 22, 3))
        noise = {k: torch.from_numpy(v[None]).to(dev) for k, v in host.items()}
        idx = torch.tensor([index], device=dev)
        rows, joints = self._sep_noise_rows(idx, noise)
        batch = self._assemble(idx, rows, joints)
        flat = torch.cat([v.reshape(-1) for v in batch.values()]).cpu().numpy()
        item, off = {}, 0
        for k, v in batch.items():
            item[k] = flat[off:off + v.numel()].reshape(tuple(v.shape[1:]))
            off += v.numel()
        return item

    def batches(self, batch_size, shuffle=False, drop_last=False, generator=None):
        """The collated batches of a `DataLoader(self, batch_size, shuffle, drop_last=drop_last)` as device float32 tensors:
        'motion_repr_clean' / 'motion_repr_noisy' [bs, clip_len-1, 294], 'noisy_joints' [bs, clip_len, 22, 3] (with
        input_noise), 'cond' [bs, clip_len-1, 22 | 13] and 'control_cond' [bs, clip_len-1, 272] (task 'traj').  shuffle
        takes a permutation from `generator` (a torch.Generator of the host or of the device; None: the default one of the
        device); with sep_noise the item noise comes from it too."""
        if not isinstance(batch_size, (int, np.integer)) or batch_size < 1:
            raise ValueError(f'batch_size must be a positive integer, got {batch_size!r}')
        n, dev, L = len(self), self.device, self.clip_len
        gdev = generator.device if generator is not None else dev
        order = torch.randperm(n, generator=generator, device=gdev).to(dev) if shuffle else torch.arange(n, device=dev)
        for a in range(0, n, batch_size):
            idx = order[a:a + batch_size]
            if drop_last and idx.shape[0] < batch_size:
                return
            if self.input_noise and self.sep_noise:
                B = int(idx.shape[0])
                shapes = {'global_orient': (B, L, 3), 'transl': (B, L, 3), 'body_pose': (B, L, 63), 'betas': (B, L, 10)}
                draw = lambda shape, scale: (torch.randn(shape, generator=generator, device=gdev, dtype=torch.float64) * scale).to(dev)
                noise = {k: draw(shapes[k], self.noise_std_params_dict[k]) for k in SEP_NOISE_ORDER}
                noise['joints'] = draw((B, L, 22, 3), self.noise_std_joint)
                yield self._assemble(idx, *self._sep_noise_rows(idx, noise))
            else:
                yield self._assemble(idx)
