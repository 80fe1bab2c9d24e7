"""Reconstruct any recording: a generic track of per-frame SMPL-X estimates instead of a PROX / EgoBody directory tree.

A track is an `.npz` file (or a dict of arrays) with one person's camera-frame estimates at any frame rate, frames where the
detector found nobody, optional 2-D keypoints and the camera's pose -- see `read_track` for the keys.  `DataloaderTrack` puts
it on the 30 fps grid the networks were trained on with one launch (`rohm_track_resample`, csrc/track.hip), marks detector
gaps as unobserved in the visibility masks instead of inventing evidence, and plans windows that cover every frame;
everything after that is `DataloaderVideo`: `frames.frames_to_world`, `clips.build_clips`, `clips.visibility_masks`.
`export.resample_params` is the way back, onto the source's own time stamps.

Limits: one person per track; `cam2world` must put the floor perpendicular to `up_axis`; there are no depth-based occlusion
masks for tracks (a user with a scene mesh can make one with `python -m rohm_amd.occlusion` and pass it as `mask_joint`)."""
from __future__ import annotations

import os

import numpy as np
import torch

from .. import _lib
from .._lib import check, lib, ptr, stream_ptr
from . import clips
from .dataloader_video import OPENPOSE_TO_SMPL, DataloaderVideo

FPS_OUT = 30.0
PARAM_COLS = {'global_orient': (0, 3), 'transl': (3, 6), 'betas': (6, 16), 'body_pose': (16, 79)}      # the project's row order
TRACK_KEYS = ('global_orient', 'transl', 'body_pose', 'betas', 'cam2world', 'fps', 'times', 'valid', 'keypoints_2d', 'mask_joint',
              'up_axis', 'focal_length', 'camera_center', 'camera_mtx', 'dist_coeffs', 'image_width', 'floor_height', 'frame_names',
              'recording_name')


# ---- the track file ------------------------------------------------------------------------------------------------------
def _scalar(v, name, typ=float):
    a = np.asarray(v)
    if a.size != 1:
        raise ValueError(f'track: {name} must be a scalar, got shape {a.shape}')
    return typ(a.reshape(-1)[0])


def read_track(path_or_dict):
    """Validate a track and return the `rec` dict `DataloaderVideo._build` consumes, plus the track's own entries.

    Required: global_orient [N,3], transl [N,3], body_pose [N,63], betas [N,10] or [10] (camera frame), cam2world [4,4] and
    exactly one of fps (times[i] = i / fps) and times [N] (seconds, strictly increasing).  Optional: valid [N] bool (a row
    with a non-finite parameter is invalid too), keypoints_2d [N,25,3] (OpenPose BODY_25, mapped through OPENPOSE_TO_SMPL)
    or [N,22,3] (SMPL order) as x, y, confidence -- without it the confidences are 1 and 2-D guidance is unavailable --,
    mask_joint [N, >=22] (default ones), up_axis 'z' | 'y' (default 'z'), focal_length [2], camera_center [2], camera_mtx
    [3,3] with dist_coeffs [5] (the keypoints are then undistorted with `clips.undistort_keypoints`) and image_width,
    floor_height, frame_names [N] (default frame_%06d), recording_name.

    Returns: 'params' (float32 dict as `read_fittings` gives it), 'params79' [N,79] float64 in the project's row order,
    'times' [N] float64, 'valid' [N] bool, 'keypoints' [N,22,3] float32, 'mask_joint' [N,M] float32, 'cam2world',
    'color_cam', 'frame_names', 'scene_name', 'recording_name', 'up_axis', 'floor_height', 'image_width',
    'has_keypoints', 'undistort'."""
    if isinstance(path_or_dict, (str, os.PathLike)):
        with np.load(path_or_dict, allow_pickle=False) as f:
            d = {k: f[k] for k in f.files}
        default_name = os.path.splitext(os.path.basename(str(path_or_dict)))[0]
    else:
        d, default_name = dict(path_or_dict), 'track'
    unknown = sorted(set(d) - set(TRACK_KEYS))
    if unknown:
        raise ValueError(f'track: unknown keys {unknown}; a track has {list(TRACK_KEYS)}')
    missing = [k for k in ('global_orient', 'transl', 'body_pose', 'betas', 'cam2world') if k not in d]
    if missing:
        raise ValueError(f'track: missing {missing}')
    go = np.asarray(d['global_orient'], dtype=np.float64)
    if go.ndim != 2 or go.shape[1] != 3 or go.shape[0] < 1:
        raise ValueError(f'track: global_orient must be [N,3] with N >= 1, got {go.shape}')
    N = go.shape[0]
    tr, bp = np.asarray(d['transl'], dtype=np.float64), np.asarray(d['body_pose'], dtype=np.float64).reshape(len(d['body_pose']), -1)
    be = np.asarray(d['betas'], dtype=np.float64)
    if be.shape == (10,):
        be = np.repeat(be[None], N, axis=0)
    if tr.shape != (N, 3) or bp.shape != (N, 63) or be.shape != (N, 10):
        raise ValueError(f'track: expected transl [{N},3], body_pose [{N},63], betas [{N},10] or [10]; got {tr.shape} {bp.shape} '
                         f'{be.shape}')
    cam2world = np.asarray(d['cam2world'], dtype=np.float64)
    if cam2world.shape != (4, 4) or not np.isfinite(cam2world).all():
        raise ValueError(f'track: cam2world must be a finite [4,4] matrix, got {cam2world.shape}')
    if ('fps' in d) == ('times' in d):
        raise ValueError('track: give exactly one of fps and times')
    if 'fps' in d:
        fps = _scalar(d['fps'], 'fps')
        if not np.isfinite(fps) or fps <= 0:
            raise ValueError(f'track: fps must be positive, got {fps}')
        times = np.arange(N, dtype=np.float64) / fps
    else:
        times = np.asarray(d['times'], dtype=np.float64)
        if times.shape != (N,):
            raise ValueError(f'track: times must be [{N}], got {times.shape}')
        if not np.isfinite(times).all() or (np.diff(times) <= 0).any():
            raise ValueError('track: times must be finite and strictly increasing')
    params79 = np.concatenate([go, tr, be, bp], axis=1)
    valid = np.ones(N, bool)
    if 'valid' in d:
        v = np.asarray(d['valid'])
        if v.shape != (N,):
            raise ValueError(f'track: valid must be [{N}], got {v.shape}')
        valid = v.astype(bool)
    valid = valid & np.isfinite(params79).all(axis=1)
    if not valid.any():
        raise ValueError('track: no valid frame (every row is marked invalid or has a non-finite parameter)')
    params79 = np.where(valid[:, None], params79, 0.0)              # rows without a fit are never read; keep them finite
    has_kp = 'keypoints_2d' in d
    if has_kp:
        kp = np.asarray(d['keypoints_2d'], dtype=np.float32)
        if kp.shape == (N, 25, 3):
            kp = kp[:, OPENPOSE_TO_SMPL[0:22]]
        elif kp.shape != (N, 22, 3):
            raise ValueError(f'track: keypoints_2d must be [{N},25,3] (BODY_25) or [{N},22,3] (SMPL order), got {kp.shape}')
        kp = np.where(np.isfinite(kp), kp, np.float32(0.0))
    else:
        kp = np.zeros((N, 22, 3), np.float32)
        kp[..., 2] = 1.0
    if 'mask_joint' in d:
        mask = np.asarray(d['mask_joint'], dtype=np.float32)
        if mask.ndim != 2 or mask.shape[0] != N or mask.shape[1] < 22:
            raise ValueError(f'track: mask_joint must be [{N}, >=22], got {mask.shape}')
    else:
        mask = np.ones((N, 22), np.float32)
    up_axis = str(np.asarray(d['up_axis']).reshape(-1)[0]) if 'up_axis' in d else 'z'
    if up_axis not in clips.UP_AXES:
        raise ValueError(f"track: up_axis must be 'z' or 'y', got {up_axis!r}")
    if ('camera_mtx' in d) != ('dist_coeffs' in d):
        raise ValueError('track: camera_mtx and dist_coeffs go together')
    color_cam = {}
    undistort = 'camera_mtx' in d
    if undistort:
        K, k = np.asarray(d['camera_mtx'], dtype=np.float64), np.asarray(d['dist_coeffs'], dtype=np.float64).reshape(-1)
        if K.shape != (3, 3) or k.shape != (5,):
            raise ValueError(f'track: camera_mtx must be [3,3] and dist_coeffs [5], got {K.shape} {k.shape}')
        color_cam.update(camera_mtx=K.tolist(), k=k.tolist(), f=[K[0, 0], K[1, 1]], c=[K[0, 2], K[1, 2]])
    for key, name in (('f', 'focal_length'), ('c', 'camera_center')):
        if name in d:
            v = np.asarray(d[name], dtype=np.float64).reshape(-1)
            if v.shape != (2,):
                raise ValueError(f'track: {name} must be [2], got {v.shape}')
            color_cam[key] = v.tolist()
    has_camera = 'f' in color_cam and 'c' in color_cam
    color_cam.setdefault('f', [0.0, 0.0])
    color_cam.setdefault('c', [0.0, 0.0])
    names = [str(s) for s in np.asarray(d['frame_names']).reshape(-1)] if 'frame_names' in d else ['frame_%06d' % i for i in range(N)]
    if len(names) != N:
        raise ValueError(f'track: frame_names must be [{N}], got {len(names)}')
    name = str(np.asarray(d['recording_name']).reshape(-1)[0]) if 'recording_name' in d else default_name
    return {'params79': params79, 'params': {k: params79[:, a:b].astype(np.float32) for k, (a, b) in PARAM_COLS.items()},
            'times': times, 'valid': valid, 'keypoints': np.ascontiguousarray(kp), 'mask_joint': np.ascontiguousarray(mask),
            'cam2world': cam2world, 'color_cam': color_cam, 'frame_names': names, 'scene_name': name, 'recording_name': name,
            'up_axis': up_axis, 'floor_height': _scalar(d['floor_height'], 'floor_height') if 'floor_height' in d else None,
            'image_width': _scalar(d['image_width'], 'image_width') if 'image_width' in d else 1920.0,
            'has_keypoints': has_kp and has_camera, 'undistort': undistort}


# ---- plans (host) --------------------------------------------------------------------------------------------------------
def plan_times(times_src, valid, fps_out=FPS_OUT):
    """The output grid: times_dst[k] = t0 + k / fps_out from the first valid source time t0 to the last valid one,
    n_out = floor((t_last - t0) * fps_out + 1e-9) + 1.  An output time that coincides with a source time bit for bit is
    copied through by the kernel: a 30 fps track that starts at 0 passes unchanged."""
    times_src, valid = np.asarray(times_src, dtype=np.float64), np.asarray(valid, dtype=bool)
    if times_src.shape != valid.shape or times_src.ndim != 1 or not valid.any():
        raise ValueError('plan_times needs times [N] and valid [N] with at least one valid frame')
    tv = times_src[valid]
    t0, t_last = float(tv[0]), float(tv[-1])
    n_out = int(np.floor((t_last - t0) * fps_out + 1e-9)) + 1
    return t0 + np.arange(n_out, dtype=np.float64) / fps_out


def plan_windows(n, clip_len, overlap_len, tail='cover'):
    """Window starts over n frames: the reference's windows every clip_len - overlap_len frames (`tail='drop'` leaves the
    frames after the last full window out, as the reference does); `tail='cover'` appends one clip starting at
    n - clip_len when frames are left over, so that every frame is in a clip."""
    if tail not in ('cover', 'drop'):
        raise ValueError(f"tail must be 'cover' or 'drop', got {tail!r}")
    nc = clips.n_clips(n, clip_len, overlap_len)
    if n < clip_len:
        raise ValueError(f'the recording has {n} frames at {FPS_OUT:g} fps; a clip needs {clip_len}: the least recording length '
                         f'is {(clip_len - 1) / FPS_OUT:.3f} s between its first and its last valid frame')
    step = clip_len - overlap_len
    starts = (np.arange(nc, dtype=np.int64) * step).tolist()
    if tail == 'cover' and starts[-1] + clip_len < n:
        starts.append(n - clip_len)
    return np.asarray(starts, dtype=np.int32)


def frames_plan(starts, rows, keep='first'):
    """Which (clip, row) every frame is exported from, for clips at explicit `starts` (ascending) holding `rows` rows each
    -> (frame_clip int32 [n], frame_t int32 [n], n_frames) as `export.plan_frames` gives it for regular windows.  A frame
    several clips share goes to the earliest (keep='first') or the latest (keep='last'); n_frames = starts[-1] + rows."""
    if keep not in ('first', 'last'):
        raise ValueError(f"keep must be 'first' or 'last', got {keep!r}")
    s = np.asarray(starts, dtype=np.int64).reshape(-1)
    rows = int(rows)
    if s.size == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), 0
    if rows < 1 or s[0] != 0 or (np.diff(s) <= 0).any():
        raise ValueError('frames_plan needs rows >= 1 and ascending starts from 0')
    n_frames = int(s[-1]) + rows
    f = np.arange(n_frames, dtype=np.int64)
    clip = np.searchsorted(s + rows, f, side='right') if keep == 'first' else np.searchsorted(s, f, side='right') - 1
    t = f - s[clip]
    if (t < 0).any() or (t >= rows).any():
        raise ValueError(f'clips of {rows} rows at starts {s.tolist()} leave frames uncovered')
    return clip.astype(np.int32), t.astype(np.int32), n_frames


# ---- the kernel's wrapper ------------------------------------------------------------------------------------------------
def _host64(x):
    return np.asarray(x.detach().cpu() if torch.is_tensor(x) else x, dtype=np.float64)


def _dev(x, dtype, device):
    if torch.is_tensor(x):
        return x.detach().to(device=device, dtype=dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype={torch.float64: np.float64, torch.float32: np.float32}[dtype])
                            ).to(device)


def default_max_gap(times_src):
    """1.5 times the median source interval: any missing source frame opens a gap."""
    t = _host64(times_src)
    return float(1.5 * np.median(np.diff(t))) if t.size > 1 else 0.0


def resample_track(times_src, valid, params, keypoints=None, mask_joint=None, times_dst=None, max_gap=None, device='cuda'):
    """`rohm_track_resample`: times_src [N], valid [N] bool, params [N,79] (float64, the project's row order), keypoints
    [N,J,3] / mask_joint [N,M] (float32, optional) as numpy arrays or device tensors -> dict of device tensors 'params'
    [n_out,79] float64, 'keypoints' [n_out,J,3] / 'mask_joint' [n_out,M] float32 (None where not given), 'src_index' int32
    and 'gap' uint8 [n_out].  times_dst defaults to `plan_times`; max_gap (seconds) to `default_max_gap`."""
    device = torch.device(device)
    if device.type != 'cuda':
        raise _lib.RohmHipError('resample_track runs on an AMD GPU; there is no CPU fallback')
    ts = _host64(times_src).reshape(-1)
    N = ts.shape[0]
    v = np.asarray(valid.detach().cpu() if torch.is_tensor(valid) else valid).astype(bool).reshape(-1)
    if N < 1 or v.shape != (N,) or not v.any():
        raise ValueError('resample_track needs times [N] and valid [N] with at least one valid frame')
    if not np.isfinite(ts).all() or (np.diff(ts) <= 0).any():
        raise ValueError('times_src must be finite and strictly increasing')
    if times_dst is None:
        times_dst = plan_times(ts, v)
    td = _host64(times_dst).reshape(-1)
    if not np.isfinite(td).all():
        raise ValueError('times_dst must be finite')
    if max_gap is None:
        max_gap = default_max_gap(ts)
    max_gap = float(max_gap)
    if not max_gap >= 0:
        raise ValueError(f'max_gap must be >= 0 seconds, got {max_gap}')
    p = _dev(params, torch.float64, device)
    if p.shape != (N, 79):
        raise ValueError(f'params must be [{N},79], got {tuple(p.shape)}')
    kp = mk = None
    J = M = 0
    if keypoints is not None:
        kp = _dev(keypoints, torch.float32, device)
        if kp.dim() != 3 or kp.shape[0] != N or kp.shape[2] != 3:
            raise ValueError(f'keypoints must be [{N},J,3], got {tuple(kp.shape)}')
        J = int(kp.shape[1])
    if mask_joint is not None:
        mk = _dev(mask_joint, torch.float32, device)
        if mk.dim() != 2 or mk.shape[0] != N:
            raise ValueError(f'mask_joint must be [{N},M], got {tuple(mk.shape)}')
        M = int(mk.shape[1])
    n_out = int(td.shape[0])
    t_src, t_dst = torch.from_numpy(ts).to(device), torch.from_numpy(np.ascontiguousarray(td)).to(device)
    vi = torch.from_numpy(np.flatnonzero(v).astype(np.int32)).to(device)
    out = {'params': torch.empty(n_out, 79, device=device, dtype=torch.float64),
           'keypoints': torch.empty(n_out, J, 3, device=device, dtype=torch.float32) if kp is not None else None,
           'mask_joint': torch.empty(n_out, M, device=device, dtype=torch.float32) if mk is not None else None,
           'src_index': torch.empty(n_out, device=device, dtype=torch.int32),
           'gap': torch.empty(n_out, device=device, dtype=torch.uint8)}
    with torch.cuda.device(device):
        check(lib().rohm_track_resample(ptr(t_src), ptr(vi), ptr(p), ptr(kp if J else None), ptr(mk if M else None), ptr(t_dst),
                                        max_gap, N, int(vi.shape[0]), J, M, n_out, ptr(out['params']),
                                        ptr(out['keypoints'] if J else None), ptr(out['mask_joint'] if M else None),
                                        ptr(out['src_index']), ptr(out['gap']), stream_ptr(device)), 'rohm_track_resample')
    return out


# ---- the dataset ---------------------------------------------------------------------------------------------------------
class DataloaderTrack(DataloaderVideo):
    """`DataloaderVideo` on a track: same items, same `batches()`.  Also: `times_src`, `valid`, `times_dst`, `src_index`, `gap`
    (host arrays; src_index / gap per 30 fps frame), `clip_starts`, and `export_plan()` for `export.export_params(plan=...)`."""

    def __init__(self, track, body_model_path='', logdir=None, task='traj', repr_abs_only=False, clip_len=150, overlap_len=2,
                 tail='cover', max_gap=None, use_scene_floor_height=False, device='cuda'):
        tr = track if isinstance(track, dict) and 'params79' in track else read_track(track)
        self._setup('track', task, repr_abs_only, clip_len, overlap_len, 22, logdir, device, use_scene_floor_height)
        self.init_root = self.base_dir = ''
        self.recording_name, self.tail = tr['recording_name'], tail
        self.up_axis, self.undistort, self.image_width = tr['up_axis'], tr['undistort'], tr['image_width']
        self.has_keypoints = tr['has_keypoints']
        self._camera(tr)
        self.scene_floor_height = tr['floor_height']
        if use_scene_floor_height and self.scene_floor_height is None:
            raise ValueError('use_scene_floor_height needs the track\'s floor_height')
        self._stats_and_model(logdir, body_model_path)
        self.times_src, self.valid = tr['times'], tr['valid']
        self.times_dst = plan_times(self.times_src, self.valid)
        self.max_gap = default_max_gap(self.times_src) if max_gap is None else float(max_gap)
        starts = plan_windows(len(self.times_dst), clip_len, overlap_len, tail)
        out = resample_track(self.times_src, self.valid, tr['params79'], tr['keypoints'], tr['mask_joint'], self.times_dst,
                             self.max_gap, self.device)
        self.src_index, self.gap = out['src_index'].cpu().numpy(), out['gap'].cpu().numpy()
        self.clip_starts = starts
        rec = {'frame_names': [tr['frame_names'][i] for i in self.src_index.tolist()], 'cam2world': tr['cam2world'],
               'params': {k: out['params'][:, a:b].float() for k, (a, b) in PARAM_COLS.items()},
               'keypoints': out['keypoints'], 'mask_joint': out['mask_joint']}
        self._build(rec, body_model_path, starts=starts)

    def export_plan(self, keep='first', rows=None):
        """(frame_clip, frame_t, n_frames) for `export.export_params(plan=...)`, the tail clip included.  rows: rows per clip
        of the representation to export (default clip_len; the drivers' pose stage keeps clip_len - 2).  keep='blend':
        `export.plan_blend`'s (frame_clip_a, frame_t_a, frame_clip_b, frame_t_b, alpha, n_frames), for a cross-fade over the
        frames two clips share."""
        if keep == 'blend':
            from ..export import plan_blend
            return plan_blend(self.clip_starts, self.clip_len if rows is None else rows)
        return frames_plan(self.clip_starts, self.clip_len if rows is None else rows, keep)
