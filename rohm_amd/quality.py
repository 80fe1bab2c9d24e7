"""Score a reconstructed track without ground truth: a per-frame report.

`drivers track` reconstructs a recording of your own and `rohm_amd.export` stitches it; this module says whether the result is
plausible and which frames to distrust.  Everything works on the stitched track -- one row per 30 fps frame, each frame
counted once -- not on clips (`rohm_scene_metrics` scores clips in canonical frames and counts overlapping frames twice).

    python -m rohm_amd.quality --saved_data_path test_results/results_track/.../walk.pkl --track walk.npz \\
        --body_model_path body_models/smplx_model --keep blend --worst 10 --json walk_quality.json --rows walk_rows.npz

Per frame (`rohm_track_quality`, csrc/quality.hip; the columns are `COLUMNS`, documented in include/rohm_hip.h): the
reprojection residual against the detected keypoints -- what the 2-D guidance optimises --, foot skating, acceleration, toe /
floor penetration and the distance to the input track, split by the input's visibility mask; the totals are split into
observed and in-filled frames (`gap`).  `floor_clearance` (`rohm_floor_clearance`) looks at the whole mesh: toes alone miss a
knee or a hand under the floor.  The scores are plausibility and consistency measures, not accuracy: a reconstruction can be
smooth, on the floor, consistent with the keypoints and still wrong."""
from __future__ import annotations

import argparse
import json
import os
import pickle
import sys

import numpy as np
import torch

from . import _lib
from ._lib import UP_AXIS, check, lib, ptr, stream_ptr, up_index as _up

COLUMNS = ('reproj_px', 'reproj_max_px', 'reproj_n', 'skate', 'accel', 'pene', 'dev_vis', 'dev_occ', 'n_vis', 'gap')
N_TOTALS = 15
GROUPS = ('observed', 'infilled')
_LOWER_IS_WORSE = ('pene',)


class TrackQuality:
    """rows [N, 10] float64 (a device tensor as `track_quality` returns it; any tensor or array works), totals [2, 15] float64
    (host; group 0 = observed frames, 1 = in-filled ones), times [N] seconds or None, clearance [N, 3] float64 or None
    (`floor_clearance` of the mesh track).  Column layouts: include/rohm_hip.h."""

    def __init__(self, rows, totals, times=None, clearance=None):
        self.rows = rows
        self.totals = np.asarray(totals, dtype=np.float64).reshape(2, N_TOTALS)
        self.times = None if times is None else np.asarray(times, dtype=np.float64).reshape(-1)
        self.clearance = clearance
        self._host = None

    def __len__(self):
        return int(self.rows.shape[0])

    def rows_host(self):
        """rows as a host array (one device-to-host copy, kept)."""
        if self._host is None:
            r = self.rows
            self._host = (r.detach().cpu().numpy() if torch.is_tensor(r) else np.asarray(r)).astype(np.float64).reshape(-1, len(COLUMNS))
        return self._host

    @staticmethod
    def _summary(s):
        with np.errstate(divide='ignore', invalid='ignore'):
            div = lambda a, b: float(np.float64(a) / np.float64(b))      # noqa: E731  (0 / 0 = nan: nothing was scored)
            return {'reproj_px': div(s[1], s[2]), 'reproj_max_px': float(s[3]), 'skating': div(s[4], s[5]), 'acc': div(s[6], s[7]),
                    'ground_pene_freq': div(s[8], s[10]) * 100.0, 'ground_pene_dist': -div(s[9], s[10]) * 1000.0,
                    'dev_vis_mm': div(s[11], s[12]) * 1000.0, 'dev_occ_mm': div(s[13], s[14]) * 1000.0,
                    'frames': int(s[0]), 'frames_reproj': int(s[2]), 'pairs_skating': int(s[5]), 'frames_acc': int(s[7]),
                    'toe_entries': int(s[10]), 'frames_dev_vis': int(s[12]), 'frames_dev_occ': int(s[14])}

    def summary(self):
        """{'observed': {...}, 'infilled': {...}, 'all': {...}}: reproj_px / reproj_max_px (pixels), skating (ratio of the
        scored pairs), acc (m/s^2), ground_pene_freq (% of toe entries more than 5 cm under the floor), ground_pene_dist (mm,
        positive) -- the names and units of `SceneMetrics.summary()` --, dev_vis_mm / dev_occ_mm (mm, against the input track)
        and the counts every mean was taken over.  NaN where nothing was scored."""
        t = self.totals
        both = t[0] + t[1]
        m = t[:, 3][~np.isnan(t[:, 3])]
        both[3] = m.max() if m.size else np.nan
        out = {g: self._summary(t[i]) for i, g in enumerate(GROUPS)}
        out['all'] = self._summary(both)
        if self.clearance is not None:
            c = self.clearance.detach().cpu().numpy() if torch.is_tensor(self.clearance) else np.asarray(self.clearance)
            gap = self.rows_host()[:, 9] != 0
            for g, sel in (('observed', ~gap), ('infilled', gap), ('all', np.ones(len(gap), bool))):
                low = c[sel, 0]
                low = low[~np.isnan(low)]
                out[g]['mesh_lowest_mm'] = float(low.min() * 1000.0) if low.size else float('nan')
                out[g]['mesh_frames_below'] = int((c[sel, 2] > 0).sum())
        return out

    _LINES = (('reproj (px)', 'reproj_px', '{:0.2f}'), ('reproj max (px)', 'reproj_max_px', '{:0.2f}'), ('skating score', 'skating', '{:0.3f}'),
              ('||acc|| (m/s^2)', 'acc', '{:0.2f}'), ('ground_pene_freq score (%)', 'ground_pene_freq', '{:0.2f}'),
              ('ground_pene_dist score (mm)', 'ground_pene_dist', '{:0.2f}'), ('dev visible (mm)', 'dev_vis_mm', '{:0.2f}'),
              ('dev occluded (mm)', 'dev_occ_mm', '{:0.2f}'), ('mesh lowest (mm)', 'mesh_lowest_mm', '{:0.1f}'),
              ('mesh frames below', 'mesh_frames_below', '{:d}'), ('frames', 'frames', '{:d}'))

    def cells(self):
        """[(label, 'observed / in-filled' text)] for the printed table."""
        s = self.summary()
        out = []
        for label, key, fmt in self._LINES:
            if key in s['observed']:
                out.append((label, ' / '.join(fmt.format(s[g][key]) for g in GROUPS)))
        return out

    def lines(self):
        """The printed form: one line per score, observed / in-filled frames."""
        return ['{:<28s} {}'.format(label + ':', text) for label, text in self.cells()]

    def worst(self, column, k=10, min_len=1):
        """The k worst contiguous frame ranges of a column (a name of `COLUMNS` or its index) as [(start, stop, peak)], stop
        exclusive, worst first.  The frame with the worst value (the largest; the most negative for 'pene') is a peak; its
        range grows over the neighbours that are at least half as bad, and stops at a NaN.  Then the same among the frames
        left, until k ranges are found or no frame is worse than 0.  Ranges shorter than min_len are dropped."""
        col = COLUMNS.index(column) if isinstance(column, str) else int(column)
        v = self.rows_host()[:, col].copy()
        if COLUMNS[col] in _LOWER_IS_WORSE:
            v = -v
        free = ~np.isnan(v)
        out = []
        while len(out) < int(k) and free.any():
            i = int(np.argmax(np.where(free, v, -np.inf)))
            peak = v[i]
            if not peak > 0:
                break
            a = b = i
            while a > 0 and free[a - 1] and v[a - 1] >= 0.5 * peak:
                a -= 1
            while b + 1 < len(v) and free[b + 1] and v[b + 1] >= 0.5 * peak:
                b += 1
            free[a:b + 1] = False
            if b + 1 - a >= int(min_len):
                out.append((a, b + 1, float(self.rows_host()[i, col])))
        return out


# ---- the kernels' wrappers -----------------------------------------------------------------------------------------------
def _tensor(x, name, shape, dtype):
    if x is None:
        return None
    if not isinstance(x, torch.Tensor):
        raise TypeError(f'{name}: track_quality takes torch tensors on a HIP device, got {type(x).__name__}')
    _lib.require_hip(x)
    if tuple(x.shape) != shape:
        raise ValueError(f'{name} must be {list(shape)}, got {list(x.shape)}')
    return x.detach().to(dtype).contiguous()


def track_quality(joints, fps=30.0, up_axis='z', floor_height=None, scene2cam=None, focal=None, center=None, keypoints=None,
                  conf_min=0.2, joints_ref=None, mask_ref=None, gap=None, times=None):
    """`rohm_track_quality` on a stitched track -> `TrackQuality`.  joints [N, 22, 3] in scene coordinates (`ExportResult.joints`
    with frame='scene'); floor_height (along up_axis; None: no skating / penetration columns); keypoints [N, 22, 3] (u, v,
    confidence, SMPL order, as `resample_track` delivers them) with scene2cam [4, 4] (inv(cam2world); array or tensor), focal
    (fx, fy) and center (cx, cy) -- all four or none; joints_ref [N, 22, 3] (the input track) and mask_ref [N, 22] (1 = the
    joint was observed); gap [N] (1 = in-filled frame).  Tensors on a HIP device only: there is no CPU path."""
    if not isinstance(joints, torch.Tensor):
        raise TypeError(f'joints: track_quality takes torch tensors on a HIP device, got {type(joints).__name__}')
    _lib.require_hip(joints)
    if joints.dim() != 3 or tuple(joints.shape[1:]) != (22, 3):
        raise ValueError(f'joints must be [N, 22, 3], got {list(joints.shape)}')
    N, dev = int(joints.shape[0]), joints.device
    up = _up(up_axis)
    fps = float(fps)
    if not (fps > 0 and np.isfinite(fps)):
        raise ValueError(f'fps must be positive, got {fps}')
    j = joints.detach().float().contiguous()
    kp = _tensor(keypoints, 'keypoints', (N, 22, 3), torch.float32)
    jr = _tensor(joints_ref, 'joints_ref', (N, 22, 3), torch.float32)
    mk = _tensor(mask_ref, 'mask_ref', (N, 22), torch.float32)
    gp = _tensor(gap, 'gap', (N,), torch.uint8)
    camera = [scene2cam is not None, focal is not None, center is not None, kp is not None]
    if any(camera) and not all(camera):
        raise ValueError('the reprojection residual needs keypoints, scene2cam, focal and center together (got %s)' %
                         ', '.join(n for n, c in zip(('scene2cam', 'focal', 'center', 'keypoints'), camera) if c))
    m = None
    fx = fy = cx = cy = 0.0
    if kp is not None:
        m = scene2cam.detach().to(device=dev, dtype=torch.float64) if torch.is_tensor(scene2cam) else \
            torch.from_numpy(np.ascontiguousarray(np.asarray(scene2cam, dtype=np.float64))).to(dev)
        if m.numel() != 16:
            raise ValueError(f'scene2cam must be [4, 4], got {list(m.shape)}')
        m = m.reshape(16).contiguous()
        (fx, fy), (cx, cy) = (float(v) for v in np.asarray(focal, dtype=np.float64).reshape(2)), \
            (float(v) for v in np.asarray(center, dtype=np.float64).reshape(2))
    has_floor = floor_height is not None
    ground = float(floor_height) if has_floor else 0.0
    if has_floor and not np.isfinite(ground):
        raise ValueError(f'floor_height must be finite, got {ground}')
    rows = torch.empty(N, len(COLUMNS), device=dev, dtype=torch.float64)
    totals = torch.zeros(2, N_TOTALS, device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        check(lib().rohm_track_quality(ptr(j), N, fps, up, int(has_floor), ground, ptr(m), fx, fy, cx, cy, ptr(kp), float(conf_min),
                                       ptr(jr), ptr(mk), ptr(gp), ptr(rows), ptr(totals), stream_ptr(dev)), 'rohm_track_quality')
    tot = totals.cpu().numpy()
    if N == 0:
        tot[:, 3] = np.nan
    return TrackQuality(rows, tot, times=times)


def floor_clearance(verts, up_axis, floor_height, below=0.05):
    """`rohm_floor_clearance`: verts [n, V, 3] float32 HIP tensor in scene coordinates -> [n, 3] float64 device tensor: the
    lowest vertex height above the floor, the index of that vertex (the lowest on ties) and the number of vertices more than
    `below` metres under the floor."""
    if not isinstance(verts, torch.Tensor):
        raise TypeError(f'verts: floor_clearance takes a torch tensor on a HIP device, got {type(verts).__name__}')
    _lib.require_hip(verts)
    if verts.dim() != 3 or verts.shape[2] != 3 or verts.shape[1] < 1:
        raise ValueError(f'verts must be [n, V >= 1, 3], got {list(verts.shape)}')
    v = verts.detach().float().contiguous()
    out = torch.empty(v.shape[0], 3, device=v.device, dtype=torch.float64)
    with torch.cuda.device(v.device):
        check(lib().rohm_floor_clearance(ptr(v), int(v.shape[0]), int(v.shape[1]), _up(up_axis), float(floor_height), float(below),
                                         ptr(out), stream_ptr(v.device)), 'rohm_floor_clearance')
    return out


# ---- a drivers' pickle -----------------------------------------------------------------------------------------------------
TRACK_PICKLE_KEYS = ('clip_starts', 'times_dst', 'gap', 'motion_repr_rec_list', 'motion_repr_noisy_list', 'trans_scene2cano_list',
                     'mask_joint_vis_list')


def load_track_pickle(pickle_or_path):
    """The dict of a `drivers track` pickle; a pickle without `clip_starts` (PROX / EgoBody / AMASS results) is refused."""
    data = pickle_or_path
    if isinstance(pickle_or_path, (str, os.PathLike)):
        with open(pickle_or_path, 'rb') as f:
            data = pickle.load(f, encoding='latin1')
    if not isinstance(data, dict) or 'clip_starts' not in data:
        raise ValueError('this is not a track pickle: it has no clip_starts, so it was not written by `python -m rohm_amd.drivers '
                         'track`.  PROX / EgoBody results have ground truth or scene metrics: score them with rohm_amd.evaluation')
    missing = [k for k in TRACK_PICKLE_KEYS if k not in data]
    if missing:
        raise ValueError(f'the track pickle has no {missing}')
    return data


def score_recording(pickle_or_path, track, body_model, keep='first', clip_len=None, vertices=False, conf_min=0.2, max_gap=None,
                    device='cuda:0'):
    """Score a `drivers track` result against the track it was made from -> {'input': TrackQuality, 'reconstruction':
    TrackQuality}, both on the stitched 30 fps rows of one export plan (the pickle's clip_starts, as `export --dataset track`
    derives it; keep = 'first' | 'last' | 'blend').  The input (`motion_repr_noisy_list`) is scored without joints_ref, the
    reconstruction (`motion_repr_rec_list`) with the input as joints_ref; mask_ref is `mask_joint_vis_list` gathered by the
    plan.  Keypoints are the track's, resampled onto the pickle's times_dst (and undistorted when the track has camera_mtx): what
    the guidance saw; give `max_gap` if the driver was given one.  Camera, up_axis and floor_height come from the track.
    clip_len: the drivers' --clip_len, checked against the pickle's rows.  vertices=True adds `floor_clearance` of both mesh
    tracks (`TrackQuality.clearance`), skinned in chunks of 256 frames."""
    from .data_loaders import clips
    from .data_loaders.track import FPS_OUT, frames_plan, read_track, resample_track
    from .export import _vertex_chunks, export_params, first_pass_rows, plan_blend
    if keep not in ('first', 'last', 'blend'):
        raise ValueError(f"keep must be 'first', 'last' or 'blend', got {keep!r}")
    data = load_track_pickle(pickle_or_path)
    tr = track if isinstance(track, dict) and 'params79' in track else read_track(track)
    device = torch.device(device)
    rec = np.asarray(data['motion_repr_rec_list'], dtype=np.float32)
    noisy = np.asarray(data['motion_repr_noisy_list'], dtype=np.float32)
    transf = np.asarray(data['trans_scene2cano_list'], dtype=np.float32)
    mask = np.asarray(data['mask_joint_vis_list'], dtype=np.float32)
    C = min(first_pass_rows(transf), len(np.asarray(data['clip_starts']).reshape(-1)))
    starts = np.asarray(data['clip_starts']).reshape(-1)[:C]
    T = rec.shape[1]
    if clip_len and not T <= int(clip_len):
        raise ValueError(f'the pickle holds {T} rows per clip, more than --clip_len {clip_len}')
    if keep == 'blend':
        plan = plan_blend(starts, T)
        plan, n = plan[:5], plan[5]
    else:
        fc, ft, n = frames_plan(starts, T, keep)
        plan = (fc, ft)
    exported = [export_params(x[:C], transf[:C], body_model, frame='scene', keep=keep, plan=plan, device=device) for x in (noisy, rec)]
    device = exported[0].joints.device
    mask_ref = torch.from_numpy(np.ascontiguousarray(mask[:C][np.asarray(plan[0]), np.asarray(plan[1])][:, :22])).to(device)
    times = np.asarray(data['times_dst'], dtype=np.float64)[:n]
    gap = torch.from_numpy(np.ascontiguousarray(np.asarray(data['gap'], dtype=np.uint8)[:n])).to(device)
    kw = dict(fps=FPS_OUT, up_axis=tr['up_axis'], floor_height=tr['floor_height'], conf_min=conf_min, mask_ref=mask_ref, gap=gap,
              times=times)
    if tr['has_keypoints']:
        kp = resample_track(tr['times'], tr['valid'], tr['params79'], tr['keypoints'], None, np.asarray(data['times_dst'], dtype=np.float64),
                            max_gap, device)['keypoints']
        if tr['undistort']:
            kp = clips.undistort_keypoints(kp, tr['color_cam']['camera_mtx'], tr['color_cam']['k'], tr['image_width'])
        kw.update(keypoints=kp[:n].contiguous(), scene2cam=np.linalg.inv(np.asarray(tr['cam2world'], dtype=np.float64)),
                  focal=tr['color_cam']['f'], center=tr['color_cam']['c'])
    out = {'input': track_quality(exported[0].joints, **kw),
           'reconstruction': track_quality(exported[1].joints, joints_ref=exported[0].joints, **kw)}
    if vertices:
        if tr['floor_height'] is None:
            raise ValueError('vertices=True measures the mesh against the floor: the track needs floor_height')
        for q, res in zip(out.values(), exported):
            parts = [floor_clearance(v, tr['up_axis'], tr['floor_height']) for _, v in _vertex_chunks(res, body_model)]
            q.clearance = torch.cat(parts, dim=0) if parts else torch.empty(0, 3, device=device, dtype=torch.float64)
    return out


# ---- the tool ----------------------------------------------------------------------------------------------------------------
def build_parser():
    ap = argparse.ArgumentParser(prog='python -m rohm_amd.quality',
                                 description='score a reconstructed track without ground truth: input against reconstruction, per frame')
    ap.add_argument('--saved_data_path', type=str, default='', help='one `drivers track` result pickle')
    ap.add_argument('--saved_data_dir', type=str, default='', help="directory of the drivers' <recording>.pkl files")
    ap.add_argument('--recordings', type=str, default='', help='comma-separated recording names (default: every pickle of the directory)')
    ap.add_argument('--track', type=str, default='', help='the track file the driver was run on (.npz)')
    ap.add_argument('--body_model_path', type=str, default='body_models/smplx_model')
    ap.add_argument('--keep', choices=['first', 'last', 'blend'], default='first', help='how the export stitches frames two clips share')
    ap.add_argument('--clip_len', type=int, default=0, help="the drivers' --clip_len (checked against the pickle)")
    ap.add_argument('--conf_min', type=float, default=0.2, help='keypoints with a confidence above this count for the residual')
    ap.add_argument('--max_gap', type=float, default=None, help="the drivers' --max_gap, if one was given")
    ap.add_argument('--vertices', action='store_true', help='also measure the whole mesh against the floor')
    ap.add_argument('--worst', type=int, default=10, help='how many worst frame ranges to list per score')
    ap.add_argument('--json', type=str, default='', help='write the summaries and worst ranges here')
    ap.add_argument('--rows', type=str, default='', help='write the per-frame rows of both tracks, times and gap here (.npz)')
    ap.add_argument('--device', type=str, default='cuda:0')
    return ap


def parse_args(argv=None):
    args = build_parser().parse_args(argv)
    if bool(args.saved_data_dir) == bool(args.saved_data_path):
        raise SystemExit('give one of --saved_data_dir and --saved_data_path')
    if not args.track:
        raise SystemExit('give --track file.npz: the camera, the keypoints and the floor come from the track')
    args.recordings = [s for s in args.recordings.split(',') if s]
    return args


def _pickles(args):
    if args.saved_data_path:
        return [args.saved_data_path]
    if args.recordings:
        return [os.path.join(args.saved_data_dir, r + '.pkl') for r in args.recordings]
    return sorted(os.path.join(args.saved_data_dir, n) for n in os.listdir(args.saved_data_dir) if n.endswith('.pkl'))


WORST_COLUMNS = ('reproj_px', 'skate', 'accel', 'pene', 'dev_vis')


def report_lines(name, scores, worst=10):
    """The printed report of one recording: a two-column table, input against reconstruction, every cell observed / in-filled
    frames; then the reconstruction's worst frame ranges per score."""
    a, b = scores['input'], scores['reconstruction']
    cells = dict(a.cells())
    out = [f'\n --------------- {name}: quality without ground truth (observed / in-filled frames) -------------',
           '{:<28s} {:>26s} {:>26s}'.format('', 'input', 'reconstruction')]
    for label, text in b.cells():
        out.append('{:<28s} {:>26s} {:>26s}'.format(label + ':', cells.get(label, 'nan / nan'), text))
    if worst > 0:
        out.append(f'worst frame ranges of the reconstruction (start, stop, peak{", seconds" if b.times is not None else ""}):')
        for col in WORST_COLUMNS:
            w = b.worst(col, worst)
            if not w:
                continue
            fmt = (lambda r: '[%d, %d) %.4g @ %.2f s' % (r[0], r[1], r[2], b.times[r[0]])) if b.times is not None else \
                (lambda r: '[%d, %d) %.4g' % r)
            out.append('  {:<10s} {}'.format(col, ', '.join(fmt(r) for r in w)))
    return out


def main(argv=None):
    args = parse_args(argv)
    loaded = []
    for p in _pickles(args):
        try:
            loaded.append((p, load_track_pickle(p)))
        except ValueError as e:
            raise SystemExit(f'{p}: {e}')
    from .data_loaders.dataloader_video import _body_model
    from .data_loaders.track import read_track
    track = read_track(args.track)
    device = torch.device(args.device)
    body = _body_model(args.body_model_path, 'neutral', device)
    notes = []
    if not track['has_keypoints']:
        notes.append('the track has no keypoints_2d (or no camera): the reprojection lines are nan')
    if track['floor_height'] is None:
        notes.append('the track has no floor_height: the skating and penetration lines are nan')
    report, rows_out = {}, {}
    for p, data in loaded:
        name = str(data.get('recording_name') or os.path.splitext(os.path.basename(p))[0])
        scores = score_recording(data, track, body, keep=args.keep, clip_len=args.clip_len or None,
                                 vertices=args.vertices and track['floor_height'] is not None, conf_min=args.conf_min, max_gap=args.max_gap,
                                 device=device)
        for line in report_lines(name, scores, args.worst):
            print(line)
        for note in notes:
            print(f'[rohm_amd.quality] note: {note}')
        report[name] = {k: {'summary': q.summary(), 'worst': {c: q.worst(c, args.worst) for c in WORST_COLUMNS}} for k, q in scores.items()}
        prefix = '' if len(loaded) == 1 else name + '/'
        rec = scores['reconstruction']
        rows_out.update({prefix + 'rows_input': scores['input'].rows_host(), prefix + 'rows_reconstruction': rec.rows_host(),
                         prefix + 'times': rec.times, prefix + 'gap': rec.rows_host()[:, 9].astype(np.uint8)})
        if rec.clearance is not None:
            rows_out.update({prefix + f'clearance_{k}': q.clearance.cpu().numpy() for k, q in scores.items()})
    if args.json:
        with open(args.json, 'w') as f:
            json.dump({'columns': list(COLUMNS), 'keep': args.keep, 'conf_min': args.conf_min, 'notes': notes, 'recordings': report}, f, indent=1)
            f.write('\n')
    if args.rows:
        np.savez(args.rows, columns=np.array(COLUMNS), **rows_out)
    return 0


if __name__ == '__main__':
    sys.exit(main())
