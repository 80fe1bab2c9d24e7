"""The result tails of the test drivers on the device.

What test_amass_full.py:387-455, test_prox_egobody.py:327-384, test_posenet.py:185-252 and test_trajnet.py:160-264 do after
every batch -- de-normalise two or three representations on the host, split them into dicts, copy them back, recover joints
(with vertices that are thrown away), copy everything to the host, re-concatenate and re-pickle all batches so far -- as
  * `result_rows`: one launch (`rohm_result_rows`) that reads the samplers' [B, 294, 1, T] outputs and the batches'
    [B, T', 294] entries in place and writes the de-normalised [B, T, 294] tensors, bit for bit the scripts' numpy values;
  * `joints_from_repr` for the joints (joints only, no vertices);
  * one `*_results` function per driver returning the batch's entries of the script's `save_data` as device tensors;
  * `ResultWriter`, which copies every saved tensor to the host once and writes the script's pickle;
  * `traj_report` / `TrajReport` / `traj_report_lines`: test_trajnet.py's report (`rohm_traj_report`).
"""
from __future__ import annotations

import math
import os
import pickle

import numpy as np
import torch

from .. import _lib
from .._lib import check, lib, ptr, stream_ptr
from ..data_loaders.motion_representation import REPR_DIM_DICT, REPR_LIST, _stats, joints_from_repr
from ..inference import ABS_TRAJ_CH, merge_traj_into_repr

ROWS_MAX = 3          # ROHM_RESULT_ROWS_MAX, include/rohm_hip.h


# ---- de-normalisation ----------------------------------------------------------------------------------------------------------
def _row_strides(x, layout):
    """(B, T, C, stride_b, stride_t, stride_c) in elements of a [B, T, C] ('btc') or [B, C, 1, T] ('bc1t') tensor."""
    if layout == 'btc' and x.dim() == 3:
        return x.shape[0], x.shape[1], x.shape[2], x.stride(0), x.stride(1), x.stride(2)
    if layout == 'bc1t' and x.dim() == 4 and x.shape[2] == 1:
        return x.shape[0], x.shape[3], x.shape[1], x.stride(0), x.stride(3), x.stride(1)
    raise ValueError(f"expected [B, T, C] ('btc') or [B, C, 1, T] ('bc1t'), got {tuple(x.shape)} as {layout!r}")


def result_rows(sources, stats, T=None):
    """De-normalise representations: `sources` is a list of (tensor, layout) or (tensor, layout, traj) with layout 'bc1t'
    ([B, C, 1, T'], the samplers' output) or 'btc' ([B, T', C]); `traj` [B, T'', 22] replaces channels 0..21 before the
    de-normalisation (test_amass_full.py:391).  `stats`: a dataset with Mean / Std, or (mean, std).  The first T frames
    (default: the first source's length) of every source are written to a new contiguous [B, T, C] float32 tensor as
    `x * Std + Mean`, two rounded float32 operations as numpy's.  Up to three sources go into one launch."""
    sources = [tuple(s) + (None,) * (3 - len(s)) for s in sources]
    if not sources:
        return []
    for x, _, traj in sources:
        if not isinstance(x, torch.Tensor) or (traj is not None and not isinstance(traj, torch.Tensor)):
            raise TypeError('result_rows takes torch tensors on a HIP device')
        _lib.require_hip(x, traj)
    dev = sources[0][0].device
    mean, std = _stats(stats, dev)
    dims = [_row_strides(x, layout) for x, layout, _ in sources]
    B, T0, Cn = dims[0][:3]
    T = T0 if T is None else int(T)
    if Cn != mean.numel():
        raise ValueError(f'{Cn} channels, but Mean / Std have {mean.numel()}')
    outs, keep = [], []
    for a in range(0, len(sources), ROWS_MAX):
        chunk = sources[a:a + ROWS_MAX]
        items = (_lib.ResultRowsItem * len(chunk))()
        for k, ((x, layout, traj), d) in enumerate(zip(chunk, dims[a:a + ROWS_MAX])):
            if d[0] != B or d[2] != Cn or d[1] < T:
                raise ValueError(f'source {a + k}: need [B={B}, T>={T}, C={Cn}], got B={d[0]} T={d[1]} C={d[2]}')
            if x.dtype != torch.float32:
                x = x.float()
                d = _row_strides(x, layout)
            rows = 0
            if traj is not None:
                if traj.dim() != 3 or traj.shape[0] != B or traj.shape[2] != 22:
                    raise ValueError(f'traj must be [{B}, T\'\', 22], got {tuple(traj.shape)}')
                traj = traj.detach().float().contiguous()
                rows = traj.shape[1]
            out = torch.empty(B, T, Cn, device=dev, dtype=torch.float32)
            items[k].src, items[k].stride_b, items[k].stride_t, items[k].stride_c = x.data_ptr(), d[3], d[4], d[5]
            items[k].mean, items[k].std = mean.data_ptr(), std.data_ptr()
            items[k].traj, items[k].traj_rows = (traj.data_ptr() if traj is not None else None), rows
            items[k].out = out.data_ptr()
            outs.append(out)
            keep.append((x, traj))          # alive until the launch is enqueued
        check(lib().rohm_result_rows(items, len(chunk), B, T, Cn, stream_ptr(dev)), 'rohm_result_rows')
    return outs


# ---- the four tails ------------------------------------------------------------------------------------------------------------
def _joints(x, mode, smplx_model):
    return joints_from_repr(x, mode, smplx_model, stats=None, layout='btc')


def amass_full_results(val_output_pose, test_batch_pose, traj_noisy_full, test_pose_dataset, smplx_model, input_noise=True):
    """test_amass_full.py:387-441 after `run_amass_iterations`: val_output_pose [bs, 294, 1, T]; test_batch_pose holds
    'motion_repr_clean' [bs, 294, 1, T] and 'motion_repr_noisy' [bs, T, 294] as the loop leaves them; traj_noisy_full
    [bs, T + 1, 22] = test_batch_traj['motion_repr_noisy'][:, :, 0:22] taken BEFORE the loop (:252).  Returns the batch's
    `save_data` arrays as device tensors, in the script's order."""
    T = val_output_pose.shape[-1]
    src = [(test_batch_pose['motion_repr_clean'], 'bc1t'), (val_output_pose, 'bc1t')]
    if input_noise:
        src.append((test_batch_pose['motion_repr_noisy'], 'btc', traj_noisy_full))
    den = result_rows(src, test_pose_dataset, T)
    clean, rec = den[0], den[1]
    out = {'rec_ric_data_clean_list': _joints(clean, 'smplx_params', smplx_model)}
    if input_noise:
        out['rec_ric_data_noisy_list'] = _joints(den[2], 'smplx_params', smplx_model)
    out['rec_ric_data_rec_list_from_abs_traj'] = _joints(rec, 'joint_abs_traj', smplx_model)
    out['rec_ric_data_rec_list_from_smpl'] = _joints(rec, 'smplx_params', smplx_model)
    out['motion_repr_clean_list'] = clean
    if input_noise:
        out['motion_repr_noisy_list'] = den[2]
    out['motion_repr_rec_list'] = rec
    return out


def posenet_results(val_output, test_batch, test_dataset, smplx_model, input_noise=True):
    """test_posenet.py:185-239: as the AMASS tail, without the trajectory override; test_batch['motion_repr_clean'] is
    [bs, 294, 1, T], test_batch['motion_repr_noisy'] [bs, T, 294]."""
    return amass_full_results(val_output, test_batch, None, test_dataset, smplx_model, input_noise)


def prox_egobody_results(val_output_joint, test_batch_pose, test_pose_dataset, smplx_model, dataset):
    """test_prox_egobody.py:327-367 after `run_prox_iterations`: val_output_joint and test_batch_pose['motion_repr_noisy']
    are [bs, 294, 1, T].  Returns the batch's `save_data` arrays (device tensors, the script's order; EgoBody's ground truth
    first) and 'frame_name_list' (the batch's names: the script saves the last batch's only, :375)."""
    if dataset not in ('prox', 'egobody'):
        raise ValueError(f"dataset must be 'prox' or 'egobody', got {dataset!r}")
    rec, noisy = result_rows([(val_output_joint, 'bc1t'), (test_batch_pose['motion_repr_noisy'], 'bc1t')], test_pose_dataset)
    out = {}
    if dataset == 'egobody':
        out['joints_gt_scene_coord_list'] = test_batch_pose['gt_joints_scene_coord']
    out['frame_name_list'] = test_batch_pose['frame_name']
    out['trans_scene2cano_list'] = test_batch_pose['transf_matrix']
    out['rec_ric_data_noisy_list'] = _joints(noisy, 'smplx_params', smplx_model)
    out['rec_ric_data_rec_list_from_abs_traj'] = _joints(rec, 'joint_abs_traj', smplx_model)
    out['rec_ric_data_rec_list_from_smpl'] = _joints(rec, 'smplx_params', smplx_model)
    out['joints_input_scene_coord_list'] = test_batch_pose['noisy_joints_scene_coord']
    out['motion_repr_noisy_list'] = noisy
    out['motion_repr_rec_list'] = rec
    out['mask_joint_vis_list'] = test_batch_pose['mask_joint_vis'][:, 0:-2, :]          # :307
    return out


def trajnet_results(val_output, test_batch, test_dataset, smplx_model, repr_abs_only=True):
    """test_trajnet.py:160-219: the clean representation with the predicted / the noisy trajectory channels put in,
    de-normalised, and the five joint recoveries.  Keys: motion_repr_clean, motion_repr_clean_root_noisy,
    motion_repr_clean_root_rec [bs, T, 294]; rec_ric_data_{clean, noisy, rec_from_abs_traj, rec_from_rel_traj, rec_from_smpl}."""
    clean_n, noisy_n = test_batch['motion_repr_clean'], test_batch['motion_repr_noisy']
    tfd = test_dataset.traj_feat_dim
    rec_n = merge_traj_into_repr(clean_n, val_output, repr_abs_only, tfd)
    traj_in = noisy_n[..., list(ABS_TRAJ_CH)] if repr_abs_only else noisy_n[:, :, 0:tfd]
    root_noisy_n = merge_traj_into_repr(clean_n, traj_in, repr_abs_only, tfd)
    clean, root_noisy, root_rec = result_rows([(clean_n, 'btc'), (root_noisy_n, 'btc'), (rec_n, 'btc')], test_dataset)
    return {'motion_repr_clean': clean, 'motion_repr_clean_root_noisy': root_noisy, 'motion_repr_clean_root_rec': root_rec,
            'rec_ric_data_clean': _joints(clean, 'smplx_params', smplx_model),
            'rec_ric_data_noisy': _joints(root_noisy, 'smplx_params', smplx_model),
            'rec_ric_data_rec_from_abs_traj': _joints(root_rec, 'joint_abs_traj', smplx_model),
            'rec_ric_data_rec_from_rel_traj': _joints(root_rec, 'joint_rel_traj', smplx_model),
            'rec_ric_data_rec_from_smpl': _joints(root_rec, 'smplx_params', smplx_model)}


# ---- the trajectory report -----------------------------------------------------------------------------------------------------
_N_REPORT = 15                                      # rohm_traj_report output layout, include/rohm_hip.h
_RECOVERIES = ('abs_traj', 'rel_traj', 'smpl')
_TRACKS = ('clean', 'noisy', 'rec_from_abs_traj', 'rec_from_rel_traj', 'rec_from_smpl')


class TrajReport:
    """Per-clip sums of `rohm_traj_report` (float64, host, [n_clip, 15]) for clips of one length.  The script's numbers are
    means over the concatenated clips, i.e. sums of these sums divided by counts: `merge` concatenates, `summary` divides."""

    def __init__(self, clip_len, sums):
        self.clip_len = int(clip_len)
        self.sums = np.asarray(sums, dtype=np.float64).reshape(-1, _N_REPORT)

    @property
    def n_clips(self):
        return len(self.sums)

    def merge(self, *others):
        for o in others:
            if o.clip_len != self.clip_len:
                raise ValueError(f'cannot merge T={o.clip_len} into T={self.clip_len}')
        return TrajReport(self.clip_len, np.concatenate([self.sums] + [o.sums for o in others], axis=0))

    def summary(self):
        """The script's names (test_trajnet.py:333-366): root_rot_err_rec (rad), root_{x,y,z}_err_rec_from_{abs_traj,
        rel_traj, smpl} (m; the script prints mm), root_pos_jitter_{clean, noisy, rec_from_*} (m/s^3)."""
        n, T = self.n_clips, self.clip_len
        s = self.sums.sum(axis=0)
        res = {'root_rot_err_rec': s[0] / (n * T)}
        for r, name in enumerate(_RECOVERIES):
            for x, axis in enumerate('xyz'):
                res[f'root_{axis}_err_rec_from_{name}'] = s[1 + r * 3 + x] / (n * T)
        for k, name in enumerate(_TRACKS):
            res['root_pos_jitter_' + name] = s[10 + k] / (n * (T - 3))
        return {k: float(v) for k, v in res.items()}

    def lines(self):
        return traj_report_lines(self.summary(), self.n_clips)


def traj_report_lines(m, n_clips):
    """The `[EVAL] ...` lines of test_trajnet.py:333-366 from the means `m` (`TrajReport.summary()`'s dict)."""
    out = ['[EVAL] {} clips in total.'.format(n_clips),
           '[EVAL] root_rot_err_rec: {:0.3f}'.format(m['root_rot_err_rec']) + ' ' +
           'degree: {:0.2f}'.format(m['root_rot_err_rec'] * 180 / math.pi)]
    for name in _RECOVERIES:
        out.append('[EVAL] root_x/y/z_err_rec_from_{} (mm): {:0.2f} / {:0.2f} / {:0.2f}'.format(
            name, *[m[f'root_{axis}_err_rec_from_{name}'] * 1000 for axis in 'xyz']))
    out.append('[EVAL] root_pos_jitter_clean / noisy / rec_from_abs_traj / rec_from_rel_traj / rec_from_smpl (m/s^3): '
               '{:0.2f} / {:0.2f} / {:0.2f} / {:0.2f} / {:0.2f}'.format(*[m['root_pos_jitter_' + k] for k in _TRACKS]))
    return out


def traj_report(joints, repr_clean, repr_rec, return_elems=False):
    """test_trajnet.py:221-263 on the device.  joints: the five [n, T, 22, 3] tensors (clean, noisy, from_abs_traj,
    from_rel_traj, from_smpl); repr_clean / repr_rec: the de-normalised [n, T, 294] representations, of which channel 0 is
    read.  One launch, one small D2H copy.  Returns a `TrajReport` (and, with `return_elems`, the float32 terms [n, 15, T]:
    rows 0..9 the errors, rows 10..14 the jitter, whose last three frames are 0)."""
    if len(joints) != 5:
        raise ValueError('traj_report takes five joint tensors: clean, noisy, from_abs_traj, from_rel_traj, from_smpl')
    for t in list(joints) + [repr_clean, repr_rec]:
        if not isinstance(t, torch.Tensor):
            raise TypeError('traj_report takes torch tensors on a HIP device')
        _lib.require_hip(t)
    js = [j.detach().float().contiguous() for j in joints]
    n, T = js[0].shape[:2]
    for j in js:
        if tuple(j.shape) != (n, T, 22, 3):
            raise ValueError(f'joints must all be [{n}, {T}, 22, 3], got {tuple(j.shape)}')
    rc, rr = repr_clean.detach().float().contiguous(), repr_rec.detach().float().contiguous()
    if rc.dim() != 3 or rc.shape[:2] != (n, T) or rr.shape != rc.shape:
        raise ValueError(f'representations must both be [{n}, {T}, C], got {tuple(rc.shape)} / {tuple(rr.shape)}')
    dev = js[0].device
    out = torch.empty(n, _N_REPORT, device=dev, dtype=torch.float64)
    elems = torch.empty(n, _N_REPORT, T, device=dev, dtype=torch.float32) if return_elems else None
    check(lib().rohm_traj_report(*[ptr(j) for j in js], ptr(rc), rc.shape[2], ptr(rr), rr.shape[2], n, T, ptr(out), ptr(elems),
                                 stream_ptr(dev)), 'rohm_traj_report')
    rep = TrajReport(T, out.cpu().numpy())
    return (rep, elems) if return_elems else rep


# ---- the pickle ----------------------------------------------------------------------------------------------------------------
def step_schedule(n_clips, batch_size):
    """Batch indices of the scripts' loop `for test_step in range(len(dataset) // batch_size + 1)` with the iterator restarted
    on exhaustion (test_amass_full.py:202-212, test_prox_egobody.py:185-195): a length that is a multiple of the batch size
    gets its first batch a second time."""
    n_batches = -(-n_clips // batch_size)
    return [k % n_batches for k in range(n_clips // batch_size + 1)] if n_batches else []


class ResultWriter:
    """Keeps the batches' `save_data` entries on the host and writes the script's pickle (protocol 2).

    `keys`: the pickle's keys in the script's order.  `static`: key -> value for the entries that are no arrays
    (`mask_scheme`, `repr_name_list`, ...).  `last_only`: keys whose value is the LAST batch's (`frame_name_list`,
    test_prox_egobody.py:375).  Every other key is the concatenation of the batches' arrays along axis 0; a key no batch
    has (e.g. the noisy entries without input noise) is left out, as in the scripts.  `add` makes one device-to-host copy
    per tensor; `write` happens after the last batch (`close`) and, with `save_interval` N > 0, after every N-th batch --
    the scripts rewrite the file after every batch, with the same final content."""

    def __init__(self, path, keys, static=None, last_only=(), save_interval=0):
        self.path, self.keys, self.static = path, list(keys), dict(static or {})
        self.last_only, self.save_interval = set(last_only), int(save_interval)
        self.batches = []

    def add(self, entries):
        unknown = [k for k in entries if k not in self.keys]
        if unknown:
            raise KeyError(f'entries {unknown} are not keys of this pickle')
        host = {}
        for k, v in entries.items():
            host[k] = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v
        self.batches.append(host)
        if self.save_interval > 0 and len(self.batches) % self.save_interval == 0:
            self.write()
        return host

    def data(self):
        out = {}
        for k in self.keys:
            if k in self.static:
                out[k] = self.static[k]
            elif k in self.last_only:
                if self.batches and k in self.batches[-1]:
                    out[k] = self.batches[-1][k]
            else:
                parts = [b[k] for b in self.batches if k in b]
                if parts:
                    out[k] = np.concatenate(parts, axis=0)
        return out

    def write(self):
        d = os.path.dirname(self.path)
        if d:
            os.makedirs(d, exist_ok=True)
        with open(self.path, 'wb') as f:
            pickle.dump(self.data(), f, protocol=2)
        return self.path

    close = write


def threshold_contact_labels(host_batch):
    """test_posenet.py:260-265: after a batch has been saved the script sets the contact channels of its `motion_repr_rec`
    and `motion_repr_clean` to 0 / 1 IN PLACE -- in the arrays its lists hold, so every later save has them thresholded for
    all batches but the newest.  Applied to a batch `ResultWriter.add` returned, before the next one is added."""
    for k in ('motion_repr_rec_list', 'motion_repr_clean_list'):
        c = host_batch[k][:, :, -4:]
        c[...] = np.where(c > 0.5, np.float32(1.0), np.float32(0.0))


AMASS_PICKLE_KEYS = ['mask_scheme', 'repr_name_list', 'repr_dim_dict', 'rec_ric_data_clean_list', 'rec_ric_data_noisy_list',
                     'rec_ric_data_rec_list_from_abs_traj', 'rec_ric_data_rec_list_from_smpl', 'motion_repr_clean_list',
                     'motion_repr_noisy_list', 'motion_repr_rec_list']                                # test_amass_full.py:443-455
POSENET_PICKLE_KEYS = AMASS_PICKLE_KEYS[1:]                                                           # test_posenet.py:241-252
SCENE_PICKLE_KEYS = ['gender_gt', 'joints_gt_scene_coord_list', 'repr_name_list', 'repr_dim_dict', 'frame_name_list',
                     'trans_scene2cano_list', 'rec_ric_data_noisy_list', 'rec_ric_data_rec_list_from_abs_traj',
                     'rec_ric_data_rec_list_from_smpl', 'joints_input_scene_coord_list', 'motion_repr_noisy_list',
                     'motion_repr_rec_list', 'mask_joint_vis_list', 'recording_name']                 # test_prox_egobody.py:369-384


def repr_static():
    return {'repr_name_list': list(REPR_LIST), 'repr_dim_dict': dict(REPR_DIM_DICT)}


# ---- file names ----------------------------------------------------------------------------------------------------------------
def amass_full_pickle_path(args):
    """test_amass_full.py:456-463."""
    save_dir = 'test_amass_full_grad_{}_mask_{}'.format(args.cond_fn_with_grad, args.mask_scheme)
    if args.input_noise and args.load_noise:
        save_dir += '_noise_{}'.format(args.load_noise_level)
    if args.infill_traj:
        save_dir += '_infill_traj_{}'.format(args.traj_mask_ratio)
    save_dir += '_iter_{}_iter2trajnoisy_{}_iter2posenoisy_{}_earlystop_{}_seed_{}.pkl'.format(
        args.sample_iter, args.iter2_cond_noisy_traj, args.iter2_cond_noisy_pose, args.early_stop, args.seed)
    return os.path.join(args.save_root, save_dir)


def prox_egobody_pickle_path(args, recording_name):
    """test_prox_egobody.py:386-390."""
    save_dir = 'test_{}_grad_{}_iter_{}_iter2trajnoisy_{}_iter2posenoisy_{}_earlystop_{}_seed_{}'.format(
        args.dataset, args.cond_fn_with_grad, args.sample_iter, args.iter2_cond_noisy_traj, args.iter2_cond_noisy_pose,
        args.early_stop, args.seed)
    return os.path.join(args.save_root, save_dir, '{}.pkl'.format(recording_name))


def posenet_pickle_path(args):
    """test_posenet.py:66-67, :253-254: next to the checkpoint."""
    log_dir = '/'.join(args.model_path.split('/')[0:-1])
    model_name = args.model_path.split('/')[-1][0:-3]
    return os.path.join(log_dir, 'test_posenet_{}_guidance_{}.pkl'.format(model_name, args.cond_fn_with_grad))
