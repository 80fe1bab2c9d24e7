"""Export a reconstruction as per-frame SMPL-X parameters and meshes in scene or camera coordinates.

The drivers leave the reference's result pickle: per clip a de-normalised 294-channel representation in the clip's own
canonical frame plus `trans_scene2cano_list`.  This module goes the other way round from the loaders
(`frames.frames_to_world` -> `clips.build_clips`): representation rows -> axis-angle SMPL-X parameters in the scene's or
the camera's frame, one track per recording, in one launch (`rohm_export_smplx`, csrc/export.hip); vertices come from the
existing skinning (`rohm_smplx_forward`) fed with the exported parameters, so they are in the chosen frame already.

    python -m rohm_amd.export --dataset prox --saved_data_dir test_results/results_prox/test_prox_... \\
        --recordings N0Sofa_00034_01 --dataset_root /data/PROX --body_model_path body_models/smplx_model \\
        --out exported --frame camera --formats npz,prox_fits --meshes ply --mesh_interval 30 --clip_len 145

Stitching: clip c holds recording frames c * (clip_len - overlap_len) ... + T - 1 (T rows per clip).  Every clip is denoised
on its own, in its own canonical frame, from its own noise, so two clips disagree on the frames they share.  `keep='first'`
(the default) takes such a frame from the earlier clip and `keep='last'` from the later one: a gather, and the body jumps at
every window boundary.  `keep='blend'` cross-fades instead (`plan_blend`, `rohm_export_smplx_blend`, the same launch that
converts the representation): over the m frames clips c - 1 and c share the weight of clip c ramps linearly as
(i + 1) / (m + 1), i = 0 .. m - 1, strictly inside (0, 1); rotations are slerped, transl / betas / contact interpolated, and
`ExportResult.disagree` keeps what the two clips disagreed by.  No frame takes more than two clips: a clip that would be the
third (heavy overlaps, the track loader's tail clip) is trimmed at its beginning.  With the reference's overlap of 2 there is
little to fade over; run the drivers with a larger `--window_size` (16 to 32 frames, about half a second to a second) when
the export is meant to be blended.  `betas='mean'`
replaces every frame's shape by the recording's mean shape before the kernel runs (so the pelvis offset and the translation
are consistent with it) -- a departure from the reference, which keeps per-frame shapes.
"""
from __future__ import annotations

import argparse
import os
import pickle
import sys

import numpy as np
import torch

from . import _lib, ops
from .body_model import lbs_forward, native_for
from ._lib import check, lib, ptr, stream_ptr

PARAM_COLS = {'global_orient': (0, 3), 'transl': (3, 6), 'betas': (6, 16), 'body_pose': (16, 79)}      # the smplx_world layout
FORMATS = ('npz', 'prox_fits')


# ---- stitching -----------------------------------------------------------------------------------------------------------
def plan_frames(n_clips, T, clip_len, overlap_len, keep='first'):
    """Which (clip, row) every recording frame is exported from -> (frame_clip int32 [n], frame_t int32 [n], n_frames).

    Clip c holds recording frames c * (clip_len - overlap_len) ... + T - 1.  A frame two clips share goes to the earlier clip
    with keep='first' and to the later one with keep='last'.  Frames after the last clip's last row are not part of the
    export: n_frames = (n_clips - 1) * (clip_len - overlap_len) + T."""
    if keep not in ('first', 'last'):
        raise ValueError(f"keep must be 'first' or 'last', got {keep!r}")
    n_clips, T, stride = int(n_clips), int(T), int(clip_len) - int(overlap_len)
    if n_clips < 0 or T < 1 or stride < 1:
        raise ValueError(f'need n_clips >= 0, T >= 1 and clip_len > overlap_len (got {n_clips}, {T}, {clip_len}, {overlap_len})')
    if n_clips > 1 and T < stride:
        raise ValueError(f'clips of {T} rows every {stride} frames leave frames uncovered')
    if n_clips == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), 0
    n_frames = (n_clips - 1) * stride + T
    f = np.arange(n_frames, dtype=np.int64)
    last = np.minimum(f // stride, n_clips - 1)
    first = np.maximum(-((-(f - T + 1)) // stride), 0)          # ceil((f - T + 1) / stride)
    clip = first if keep == 'first' else last
    return clip.astype(np.int32), (f - clip * stride).astype(np.int32), n_frames


def plan_blend(starts, rows):
    """The cross-fade plan for clips at ascending `starts` (starts[0] == 0) holding `rows` rows each ->
    (frame_clip_a, frame_t_a, frame_clip_b, frame_t_b int32 [n], alpha float64 [n], n_frames), n_frames = starts[-1] + rows.

    With hi_c = starts[c] + rows the active range of clip c is [lo_c, hi_c): lo_0 = 0, lo_1 = starts[1] and
    lo_c = max(starts[c], hi_{c-2}) for c >= 2, so no frame is in the active range of more than two clips (a clip that would
    be the third is trimmed at its beginning: its own edge rows).  A frame f in [lo_c, hi_{c-1}) is shared by a = c - 1 and
    b = c with alpha = (i + 1) / (m + 1), m = hi_{c-1} - lo_c, i = f - lo_c: the weight of b, a linear ramp strictly inside
    (0, 1).  Every other frame belongs to one clip: frame_clip_b = -1, frame_t_b = 0, alpha = 0.  Rows are f - starts[clip].
    Regular windows: starts = arange(C) * (clip_len - overlap_len)."""
    s = np.asarray(starts, dtype=np.int64).reshape(-1)
    rows = int(rows)
    if s.size == 0:
        z = np.zeros(0, np.int32)
        return z, z.copy(), z.copy(), z.copy(), np.zeros(0, np.float64), 0
    if rows < 1 or s[0] != 0 or (np.diff(s) <= 0).any():
        raise ValueError('plan_blend needs rows >= 1 and ascending starts from 0')
    hi = s + rows
    if (s[1:] > hi[:-1]).any():
        raise ValueError(f'clips of {rows} rows at starts {s.tolist()} leave frames uncovered')
    lo = s.copy()
    lo[2:] = np.maximum(s[2:], hi[:-2])
    n_frames = int(hi[-1])
    clip_a, clip_b = np.zeros(n_frames, np.int64), np.full(n_frames, -1, np.int64)
    alpha = np.zeros(n_frames, np.float64)
    for c in range(1, len(s)):
        clip_a[hi[c - 1]:hi[c]] = c                                  # until clip c + 1 takes over, clip c alone
        m = int(hi[c - 1] - lo[c])
        if m > 0:
            clip_b[lo[c]:hi[c - 1]] = c
            alpha[lo[c]:hi[c - 1]] = (np.arange(m, dtype=np.float64) + 1.0) / (m + 1.0)
    f = np.arange(n_frames, dtype=np.int64)
    t_a = f - s[clip_a]
    t_b = np.where(clip_b >= 0, f - s[np.maximum(clip_b, 0)], 0)
    return clip_a.astype(np.int32), t_a.astype(np.int32), clip_b.astype(np.int32), t_b.astype(np.int32), alpha, n_frames


def first_pass_rows(trans_scene2cano):
    """Rows of a drivers' pickle that belong to the first pass over the recording.  The drivers' batch loop restarts its
    loader when it runs out (`drivers.results.step_schedule`): a clip count that is a multiple of the batch size gets its first
    batch a second time.  The first row r >= 1 whose trans_scene2cano equals row 0's bit for bit starts that repeat."""
    a = np.ascontiguousarray(np.asarray(trans_scene2cano))
    for r in range(1, len(a)):
        if a[r].tobytes() == a[0].tobytes():
            return r
    return len(a)


# ---- the export ----------------------------------------------------------------------------------------------------------
class ExportResult:
    """Device tensors of an exported track: params79 [N, 79] float64 (global_orient 3, transl 3, betas 10, body_pose 63) and its
    four views, joints [N, 22, 3] float32, contact [N, 4] float32, frame_clip / frame_t int32 [N], coordinate_frame.
    A blended export (keep='blend') also has frame_clip_b / frame_t_b int32 [N] (-1 / 0 where one clip gave the frame), alpha
    float64 [N] (the weight of clip b) and disagree [N, 23] float64: the geodesic angle (rad) between the two clips' rotations
    per joint and, in column 22, the distance (m) between their pelvis positions; they are None otherwise."""

    def __init__(self, params79, joints, contact, frame_clip, frame_t, coordinate_frame, times=None, gap=None, frame_clip_b=None,
                 frame_t_b=None, alpha=None, disagree=None):
        self.params79, self.joints, self.contact = params79, joints, contact
        self.frame_clip, self.frame_t, self.coordinate_frame = frame_clip, frame_t, coordinate_frame
        self.times, self.gap = times, gap          # tracks: seconds [N] float64 and "no evidence here" [N] uint8 (host arrays)
        self.frame_clip_b, self.frame_t_b, self.alpha, self.disagree = frame_clip_b, frame_t_b, alpha, disagree
        for k, (a, b) in PARAM_COLS.items():
            setattr(self, k, params79[:, a:b])

    def __len__(self):
        return int(self.params79.shape[0])

    def pose_f32(self):
        """[N, 22, 3] float32 axis-angle, global orient first (what rohm_smplx_joints / rohm_smplx_forward take)."""
        return torch.cat([self.global_orient, self.body_pose], dim=1).float().reshape(-1, 22, 3).contiguous()


def _device_f32(x, device):
    if torch.is_tensor(x):
        return x.detach().to(device=device, dtype=torch.float32)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.float32)).to(device)


def _layout(x):
    if x.dim() == 3 and x.shape[2] == 294:
        return 'btc', x.shape[0], x.shape[1]
    if x.dim() == 4 and x.shape[1] == 294 and x.shape[2] == 1:
        return 'bc1t', x.shape[0], x.shape[3]
    raise ValueError(f'expected [C, T, 294] or [C, 294, 1, T], got {tuple(x.shape)}')


def _joints(nat, pose, betas, transl):
    N = pose.shape[0]
    out = torch.empty(N, 22, 3, device=pose.device, dtype=torch.float32)
    if N:
        check(lib().rohm_smplx_joints(nat.handle, ptr(pose), 22, ptr(betas), ptr(transl), N, ptr(out), 22, stream_ptr(pose.device)),
              'rohm_smplx_joints')
    return out


def export_params(repr, transf, body_model, clip_len=None, overlap_len=2, frame='scene', cam2world=None, betas='frame',
                  stats=None, keep='first', plan=None, device=None):
    """Representation rows -> an `ExportResult` of per-frame SMPL-X parameters in scene or camera coordinates.

    repr: [C, T, 294] or the networks' [C, 294, 1, T] (read in place), a device tensor straight from
    `prox_egobody_results` / `run_prox_iterations` or an array from a pickle; `stats` = (mean, std) or a dataset with Mean / Std
    when it is still normalised.  transf [C, 4, 4]: scene -> canonical (`trans_scene2cano_list`, `transf_matrix`), None for
    clips that stay in their canonical frame.  frame='camera' applies inv(cam2world) after the way back to the scene.
    clip_len defaults to T + 1 (the loaders' clips); `plan` = (frame_clip, frame_t) overrides `plan_frames`.
    keep='blend' cross-fades the frames two clips share (`plan_blend`, one launch of `rohm_export_smplx_blend`); `plan` may
    then be the 5 arrays of a blend plan (frame_clip_a, frame_t_a, frame_clip_b, frame_t_b, alpha), and a plan of 5 arrays
    blends whatever `keep` says.  keep='first' / 'last' run `rohm_export_smplx` as before.
    betas='mean' exports the recording's mean shape for every frame (not what the reference does: it keeps per-frame shapes);
    in a blended export the mean is taken over the candidate-a rows."""
    if keep not in ('first', 'last', 'blend'):
        raise ValueError(f"keep must be 'first', 'last' or 'blend', got {keep!r}")
    if frame not in ('scene', 'camera'):
        raise ValueError(f"frame must be 'scene' or 'camera', got {frame!r}")
    if betas not in ('frame', 'mean'):
        raise ValueError(f"betas must be 'frame' or 'mean', got {betas!r}")
    if frame == 'camera' and cam2world is None:
        raise ValueError("frame='camera' needs cam2world")
    if device is None:
        device = repr.device if torch.is_tensor(repr) and repr.is_cuda else body_model.v_template.device
    device = torch.device(device)
    nat = native_for(body_model, device)
    device = nat.device
    x = _device_f32(repr, device)
    layout, C, T = _layout(x)
    tf = None if transf is None else _device_f32(transf, device).reshape(C, 4, 4).contiguous()
    rigid = None
    if frame == 'camera':
        inv = np.linalg.inv(np.asarray(cam2world.detach().cpu() if torch.is_tensor(cam2world) else cam2world, dtype=np.float64))
        rigid = torch.from_numpy(np.ascontiguousarray(inv.reshape(4, 4))).to(device)
    if plan is None and keep == 'blend':
        stride = (T + 1 if clip_len is None else int(clip_len)) - int(overlap_len)
        if stride < 1:
            raise ValueError(f'need clip_len > overlap_len (got {clip_len}, {overlap_len})')
        plan = plan_blend(np.arange(C, dtype=np.int64) * stride, T)[:5]
    elif plan is None:
        plan = plan_frames(C, T, T + 1 if clip_len is None else clip_len, overlap_len, keep)[:2]
    plan = tuple(plan)
    blend = len(plan) >= 5
    if keep == 'blend' and not blend:
        raise ValueError("keep='blend' needs the 5 arrays of `plan_blend` as plan, got %d" % len(plan))

    def index(a, dtype, np_dtype):
        a = a.to(device, dtype) if torch.is_tensor(a) else torch.as_tensor(np.asarray(a, dtype=np_dtype)).to(device)
        return a.contiguous()
    fc, ft = index(plan[0], torch.int32, np.int32), index(plan[1], torch.int32, np.int32)
    mean = std = None
    if stats is not None:
        from .data_loaders.motion_representation import _stats
        mean, std = _stats(stats, device)
    if betas == 'mean' and fc.numel():
        # the kernel must see the mean shape: de-normalise once (rohm_result_rows: the same two float32 operations), overwrite
        from .drivers.results import result_rows
        if mean is not None:
            x = result_rows([(x, layout)], stats)[0]
        else:
            x = (x if layout == 'btc' else x[:, :, 0].permute(0, 2, 1)).contiguous().clone()
        layout, mean, std = 'btc', None, None
        ok = (fc >= 0) & (fc < C) & (ft >= 0) & (ft < T)
        rows = x[fc[ok].long(), ft[ok].long(), 280:290]
        x[:, :, 280:290] = rows.double().mean(dim=0).float()
    if blend:
        fcb, ftb, al = index(plan[2], torch.int32, np.int32), index(plan[3], torch.int32, np.int32), index(plan[4], torch.float64, np.float64)
        params, contact, disagree = ops.export_smplx_blend(nat.handle, x, layout, fc, ft, fcb, ftb, al, transf=tf, rigid=rigid, mean=mean,
                                                           std=std)
        res = ExportResult(params, None, contact, fc, ft, frame, frame_clip_b=fcb, frame_t_b=ftb, alpha=al, disagree=disagree)
    else:
        params, contact = ops.export_smplx(nat.handle, x, layout, fc, ft, transf=tf, rigid=rigid, mean=mean, std=std)
        res = ExportResult(params, None, contact, fc, ft, frame)
    res.joints = _joints(nat, res.pose_f32(), res.betas.float().contiguous(), res.transl.float().contiguous())
    return res


def resample_params(result, times_from, times_to, body_model=None, gap_from=None, max_gap=None):
    """An exported track on other time stamps: `rohm_track_resample` (csrc/track.hip) with J = M = 0 on params79, every row of
    `result` valid.  times_from [N]: the times of the rows of `result` (a `DataloaderTrack`'s times_dst); times_to [n]: e.g. the
    source's own time stamps.  Rotations are slerped, transl and betas interpolated, a time that coincides with one of
    times_from is that row's bits; contact, frame_clip and frame_t are those of the row at the left bracket.  With `body_model`
    the joints are recomputed from the new parameters (`rohm_smplx_joints`).  The result carries `times` = times_to and `gap`
    [n] uint8: 1 where times_to lies outside times_from (the nearest row is held), where the brackets are further apart
    than max_gap (default 1.5 intervals of times_from) or where `gap_from` [N] is set at the left bracket.  A blended
    export's frame_clip_b, frame_t_b, alpha and disagree are those of the row at the left bracket too."""
    from .data_loaders.track import resample_track
    tf = np.asarray(times_from, dtype=np.float64).reshape(-1)
    tt = np.asarray(times_to, dtype=np.float64).reshape(-1)
    if tf.shape[0] != len(result):
        raise ValueError(f'{len(result)} exported rows but {tf.shape[0]} times')
    device = result.params79.device
    out = resample_track(tf, np.ones(tf.shape[0], bool), result.params79, None, None, tt, max_gap, device)
    left = out['src_index'].long()
    gap = out['gap'].cpu().numpy()
    if gap_from is not None:
        gap = gap | np.asarray(gap_from, dtype=np.uint8).reshape(-1)[out['src_index'].cpu().numpy()]
    res = ExportResult(out['params'], None, result.contact[left] if result.contact is not None else None, result.frame_clip[left],
                       result.frame_t[left], result.coordinate_frame, times=tt, gap=gap)
    res.src_index = out['src_index']
    if result.disagree is not None:
        res.frame_clip_b, res.frame_t_b, res.alpha, res.disagree = (getattr(result, k)[left] for k in ('frame_clip_b', 'frame_t_b', 'alpha',
                                                                                                      'disagree'))
    if body_model is not None:
        nat = native_for(body_model, device)
        res.joints = _joints(nat, res.pose_f32(), res.betas.float().contiguous(), res.transl.float().contiguous())
    return res


def _vertex_chunks(result, body_model, every=1, chunk=256):
    """Yields (frame indices, verts [n, V, 3] float32 device tensor) over the frames 0, every, 2 every, ..."""
    nat = native_for(body_model, result.params79.device)
    idx = torch.arange(0, len(result), max(int(every), 1), device=result.params79.device)
    pose, be, tr = result.pose_f32(), result.betas.float(), result.transl.float()
    for a in range(0, idx.numel(), chunk):
        sel = idx[a:a + chunk]
        _, verts = lbs_forward(nat, pose[sel].contiguous(), 0, be[sel].contiguous(), tr[sel].contiguous())
        yield sel, verts


def export_vertices(result, body_model, every=1, chunk=256):
    """Vertices [ceil(N / every), V, 3] (float32, device) of every `every`-th exported frame: `rohm_smplx_forward` with
    axis-angle poses on the exported parameters, in chunks -- already in the export's coordinate frame."""
    parts = [v for _, v in _vertex_chunks(result, body_model, every, chunk)]
    if not parts:
        nat = native_for(body_model, result.params79.device)
        return torch.empty(0, nat.num_verts, 3, device=result.params79.device, dtype=torch.float32)
    return torch.cat(parts, dim=0)


def seam_summary(result):
    """(number of seams, largest seam_angle in rad, largest seam_dist in m) of a blended export; a seam is a pair of clips
    that share frames."""
    b = _host(result.frame_clip_b).reshape(-1)
    if not (b >= 0).any():
        return 0, 0.0, 0.0
    pairs = np.stack([_host(result.frame_clip).reshape(-1)[b >= 0], b[b >= 0]], axis=1)
    dis = _host(result.disagree).reshape(-1, 23)[b >= 0]
    return len(np.unique(pairs, axis=0)), float(dis[:, :22].max()), float(dis[:, 22].max())


# ---- writers (host) ----------------------------------------------------------------------------------------------------------
def _host(t, dtype=None):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return a if dtype is None else a.astype(dtype)


def _names(frame_names, n):
    names = [str(s) for s in frame_names]
    if len(names) < n:
        raise ValueError(f'{n} frames but {len(names)} frame names')
    return names[:n]


def write_npz(path, result, frame_names):
    """One smplx_params.npz per recording: global_orient / transl / betas / body_pose (float32), joints, foot_contact,
    frame_names, frame_clip, coordinate_frame, gender; for a track also times (seconds) and gap (1 = no evidence at this frame);
    for a blended export also frame_clip_b (-1: one clip), blend_alpha, seam_angle (rad: the largest of the 22 joints' geodesic
    angles between the two clips) and seam_dist (m, between their pelvis positions)."""
    p = _host(result.params79)
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    out = {k: p[:, a:b].astype(np.float32) for k, (a, b) in PARAM_COLS.items()}
    if getattr(result, 'times', None) is not None:
        out['times'] = np.asarray(result.times, dtype=np.float64)
    if getattr(result, 'gap', None) is not None:
        out['gap'] = np.asarray(result.gap, dtype=np.uint8)
    if getattr(result, 'disagree', None) is not None:
        dis = _host(result.disagree, np.float64).reshape(len(p), 23)
        out.update(frame_clip_b=_host(result.frame_clip_b, np.int32), blend_alpha=_host(result.alpha, np.float64),
                   seam_angle=dis[:, :22].max(axis=1) if len(p) else np.zeros(0), seam_dist=dis[:, 22])
    np.savez(path, joints=_host(result.joints, np.float32), foot_contact=_host(result.contact, np.float32),
             frame_names=np.array(_names(frame_names, len(p))), frame_clip=_host(result.frame_clip, np.int32),
             coordinate_frame=np.str_(result.coordinate_frame), gender=np.str_('neutral'), **out)
    return path


def write_prox_fits(root, recording, result, frame_names, body_idx=None):
    """<root>/<recording>/results/<frame>/000.pkl (EgoBody's layout with `body_idx`: <root>/<recording>/body_idx_<k>/results/...)
    with the keys the loaders read -- transl, global_orient, betas, body_pose, each [1, k] float32 -- and zero jaw_pose,
    leye_pose, reye_pose, expression.  The loaders expect camera coordinates: export with frame='camera'."""
    p = _host(result.params79).astype(np.float32)
    base = os.path.join(root, recording) if body_idx is None else os.path.join(root, recording, f'body_idx_{body_idx}')
    zeros = {'jaw_pose': 3, 'leye_pose': 3, 'reye_pose': 3, 'expression': 10}
    for i, name in enumerate(_names(frame_names, len(p))):
        d = os.path.join(base, 'results', name)
        os.makedirs(d, exist_ok=True)
        row = {k: p[i:i + 1, a:b].copy() for k, (a, b) in PARAM_COLS.items()}
        row.update({k: np.zeros((1, n), np.float32) for k, n in zeros.items()})
        with open(os.path.join(d, '000.pkl'), 'wb') as f:
            pickle.dump(row, f, protocol=2)
    return os.path.join(base, 'results')


def write_ply(path, verts, faces):
    """Binary little-endian PLY (float x y z, uchar-counted int faces) that `rohm_amd.occlusion.read_ply` reads back."""
    v = np.ascontiguousarray(_host(verts), dtype='<f4').reshape(-1, 3)
    f = np.asarray(_host(faces)).reshape(-1, 3)
    rec = np.zeros(len(f), dtype=np.dtype([('n', 'u1'), ('v', '<i4', (3,))]))
    rec['n'], rec['v'] = 3, f
    head = ('ply\nformat binary_little_endian 1.0\nelement vertex {}\nproperty float x\nproperty float y\nproperty float z\n'
            'element face {}\nproperty list uchar int vertex_indices\nend_header\n').format(len(v), len(f))
    with open(path, 'wb') as out:
        out.write(head.encode('ascii'))
        out.write(v.tobytes())
        out.write(rec.tobytes())
    return path


def write_obj(path, verts, faces):
    v = _host(verts).reshape(-1, 3)
    f = np.asarray(_host(faces)).reshape(-1, 3) + 1
    with open(path, 'w') as out:
        out.writelines('v {:.8g} {:.8g} {:.8g}\n'.format(*r) for r in v.tolist())
        out.writelines('f {} {} {}\n'.format(*r) for r in f.tolist())
    return path


def write_meshes(out_dir, result, body_model, frame_names, mesh_interval=1, fmt='ply', chunk=256):
    """meshes/<frame>.ply (or .obj) for every `mesh_interval`-th frame; one device-to-host copy per chunk of meshes."""
    faces = getattr(body_model, 'faces', None)
    if faces is None:
        raise _lib.RohmHipError("meshes need the body model's faces (SMPLXLayer.from_npz keeps them)")
    faces = np.asarray(faces).astype(np.int32).reshape(-1, 3)
    names = _names(frame_names, len(result))
    d = os.path.join(out_dir, 'meshes')
    os.makedirs(d, exist_ok=True)
    write = write_ply if fmt == 'ply' else write_obj
    n = 0
    for sel, verts in _vertex_chunks(result, body_model, mesh_interval, chunk):
        host = verts.cpu().numpy()
        for i, v in zip(sel.tolist(), host):
            write(os.path.join(d, f'{names[i]}.{fmt}'), v, faces)
            n += 1
    return n


# ---- the tool -----------------------------------------------------------------------------------------------------------------
def build_parser():
    ap = argparse.ArgumentParser(prog='python -m rohm_amd.export',
                                 description='SMPL-X parameters and meshes of a reconstruction, in scene or camera coordinates')
    ap.add_argument('--dataset', choices=['prox', 'egobody', 'amass', 'track'], default='prox')
    ap.add_argument('--saved_data_dir', type=str, default='', help='directory of the drivers\' <recording>.pkl files')
    ap.add_argument('--saved_data_path', type=str, default='', help='one result pickle')
    ap.add_argument('--recordings', type=str, default='', help='comma-separated recording names (default: every pickle of the directory)')
    ap.add_argument('--dataset_root', type=str, default='', help='PROX / EgoBody root (calibration; needed for --frame camera)')
    ap.add_argument('--body_model_path', type=str, default='body_models/smplx_model')
    ap.add_argument('--out', type=str, default='exported')
    ap.add_argument('--frame', choices=['scene', 'camera'], default='scene')
    ap.add_argument('--formats', type=str, default='npz', help='comma-separated: npz, prox_fits')
    ap.add_argument('--meshes', choices=['none', 'ply', 'obj'], default='none')
    ap.add_argument('--mesh_interval', type=int, default=1)
    ap.add_argument('--keep', choices=['first', 'last', 'blend'], default='first',
                    help='a frame two clips share: from the earlier clip, from the later one, or a cross-fade of both')
    ap.add_argument('--betas', choices=['frame', 'mean'], default='frame')
    ap.add_argument('--overlap_len', type=int, default=2)
    ap.add_argument('--clip_len', type=int, default=0, help='frames per loader clip; 0 = rows per clip + 1.  The drivers\' pose '
                    'stage keeps clip_len - 2 rows: give their --clip_len for their pickles')
    ap.add_argument('--init_root', type=str, default='', help='initial fits: frame names come from its sorted listing')
    ap.add_argument('--times', choices=['source', '30fps'], default='source',
                    help='--dataset track: export on the source\'s own time stamps or on the 30 fps grid of the reconstruction')
    ap.add_argument('--device', type=str, default='cuda:0')
    return ap


def parse_args(argv=None):
    args = build_parser().parse_args(argv)
    args.formats = [s for s in args.formats.split(',') if s]
    bad = [s for s in args.formats if s not in FORMATS]
    if bad:
        raise SystemExit(f'--formats: unknown {bad}; choose from {list(FORMATS)}')
    args.recordings = [s for s in args.recordings.split(',') if s]
    if bool(args.saved_data_dir) == bool(args.saved_data_path):
        raise SystemExit('give one of --saved_data_dir and --saved_data_path')
    if args.frame == 'camera' and args.dataset != 'track' and (args.dataset == 'amass' or not args.dataset_root):
        raise SystemExit('--frame camera needs --dataset prox|egobody and --dataset_root (the calibration files)')
    return args


def _pickles(args):
    if args.saved_data_path:
        return [args.saved_data_path]
    if args.recordings:
        return [os.path.join(args.saved_data_dir, r + '.pkl') for r in args.recordings]
    return sorted(os.path.join(args.saved_data_dir, n) for n in os.listdir(args.saved_data_dir) if n.endswith('.pkl'))


def _frame_names(args, recording, info, n):
    if args.init_root and args.dataset in ('prox', 'egobody'):
        sub = (recording, 'results') if args.dataset == 'prox' else (recording, f"body_idx_{info['body_idx']}", 'results')
        names = sorted(os.listdir(os.path.join(args.init_root, *sub)))
        if len(names) >= n:
            return names[:n]
        print(f'[rohm_amd.export] {recording}: {len(names)} frame folders for {n} frames, numbering them instead')
    return ['frame_%05d' % i for i in range(n)]


def _export_one(args, path, body, device):
    with open(path, 'rb') as f:
        data = pickle.load(f, encoding='latin1')
    rec = np.asarray(data['motion_repr_rec_list'], dtype=np.float32)
    n_written = 0
    if args.dataset == 'amass':
        T = rec.shape[1]
        base = os.path.splitext(os.path.basename(path))[0]
        rec = torch.from_numpy(rec).to(device)
        for c in range(rec.shape[0]):
            plan = (np.full(T, c, np.int32), np.arange(T, dtype=np.int32))
            res = export_params(rec, None, body, frame='scene', betas=args.betas, plan=plan, device=device)
            out = os.path.join(args.out, base, 'seq_%03d' % c)
            names = ['frame_%05d' % i for i in range(T)]
            n_written += _write(args, out, 'seq_%03d' % c, res, body, names, None)
        return n_written
    recording = str(data.get('recording_name') or os.path.splitext(os.path.basename(path))[0])
    transf = np.asarray(data['trans_scene2cano_list'], dtype=np.float32)
    keep_rows = first_pass_rows(transf)
    if keep_rows < len(transf):
        print(f'[rohm_amd.export] {recording}: rows {keep_rows}..{len(transf) - 1} repeat the first batch, dropped')
        rec, transf = rec[:keep_rows], transf[:keep_rows]
    if args.dataset == 'track':
        return _export_track(args, data, rec, transf, recording, body, device)
    info, cam2world = None, None
    if args.dataset == 'egobody' and args.dataset_root:
        from .data_loaders.dataloader_video import read_egobody_info
        info = read_egobody_info(args.dataset_root, recording)
    if args.frame == 'camera':
        from .data_loaders.dataloader_video import read_cam2world
        cam2world = read_cam2world(args.dataset, args.dataset_root, recording, info)
    T = rec.shape[1]
    res = export_params(rec, transf, body, clip_len=args.clip_len or T + 1, overlap_len=args.overlap_len, frame=args.frame,
                        cam2world=cam2world, betas=args.betas, keep=args.keep, device=device)
    if args.dataset == 'egobody' and info is None and (args.init_root or 'prox_fits' in args.formats):
        raise SystemExit('EgoBody frame names and fit folders need --dataset_root (egobody_rohm_info.csv)')
    names = _frame_names(args, recording, info, len(res))
    return _write(args, os.path.join(args.out, recording), recording, res, body, names, info)


def _export_track(args, data, rec, transf, recording, body, device):
    """A `drivers track` pickle: the plan, the times and the camera come from the pickle itself."""
    from .data_loaders.track import frames_plan
    missing = [k for k in ('clip_starts', 'times_dst', 'src_index', 'gap', 'times_src', 'valid', 'source_frame_names', 'cam2world')
               if k not in data]
    if missing:
        raise SystemExit(f'--dataset track: the pickle has no {missing}; it was not written by `python -m rohm_amd.drivers track`')
    starts = np.asarray(data['clip_starts']).reshape(-1)[:len(rec)]
    if args.keep == 'blend':
        plan = plan_blend(starts, rec.shape[1])
        plan, n = plan[:5], plan[5]
    else:
        fc, ft, n = frames_plan(starts, rec.shape[1], args.keep)
        plan = (fc, ft)
    res = export_params(rec[:len(starts)], transf[:len(starts)], body, frame=args.frame, cam2world=np.asarray(data['cam2world']),
                        betas=args.betas, keep=args.keep, plan=plan, device=device)
    times30, gap30 = np.asarray(data['times_dst'], dtype=np.float64)[:n], np.asarray(data['gap'], dtype=np.uint8)[:n]
    src_names = [str(s) for s in data['source_frame_names']]
    if args.times == '30fps':
        res.times, res.gap = times30, gap30
        names = [src_names[i] for i in np.asarray(data['src_index'])[:n].tolist()]          # the source frame at the left bracket
        if len(set(names)) < len(names):
            names = ['%s_%06d' % (s, k) for k, s in enumerate(names)]
    else:
        # one row per source frame between the first and the last frame that had a fit, the frames without one included; a
        # source time after the last reconstructed row (the pose stage keeps clip_len - 2 rows) holds that row, gap = 1
        v = np.flatnonzero(np.asarray(data['valid'], dtype=bool))
        sel = slice(int(v[0]), int(v[-1]) + 1)
        res = resample_params(res, times30, np.asarray(data['times_src'], dtype=np.float64)[sel], body, gap_from=gap30)
        names = src_names[sel]
    return _write(args, os.path.join(args.out, recording), recording, res, body, names, None)


def _write(args, out, recording, res, body, names, info):
    os.makedirs(out, exist_ok=True)
    if 'npz' in args.formats:
        write_npz(os.path.join(out, 'smplx_params.npz'), res, names)
    if 'prox_fits' in args.formats:
        write_prox_fits(os.path.join(out, 'fits'), recording, res, names, body_idx=info['body_idx'] if info else None)
    n_mesh = 0
    if args.meshes != 'none':
        n_mesh = write_meshes(out, res, body, names, args.mesh_interval, args.meshes)
    print(f'[rohm_amd.export] {recording}: {len(res)} frames ({res.coordinate_frame}), {n_mesh} meshes -> {out}')
    if res.disagree is not None:
        n_seams, angle, dist = seam_summary(res)
        print(f'[rohm_amd.export] {recording}: {n_seams} seams blended, largest seam_angle {angle:.4f} rad, largest seam_dist {dist:.4f} m')
    return len(res)


def main(argv=None):
    args = parse_args(argv)
    from .data_loaders.dataloader_video import _body_model
    device = torch.device(args.device)
    body = _body_model(args.body_model_path, 'neutral', device)
    total = sum(_export_one(args, p, body, device) for p in _pickles(args))
    print(f'[rohm_amd.export] {total} frames exported')
    return 0


if __name__ == '__main__':
    sys.exit(main())
