"""Native `preprocessing_amass.py`: raw AMASS (SMPL-X neutral .npz recordings) -> the 30 fps trees the AMASS loader reads.

`python -m rohm_amd.preprocessing_amass --body_model_path ... --amass_root ... --dataset_name ACCAD --save_root ...` writes what
the reference script writes: `pose_data_fps_30/<dataset>/<subject>/<recording>.npy` (float32 [n, 25, 3]: joints 0..24 of the
neutral SMPL-X body) and `smpl_data_fps_30/<dataset>/<subject>/<recording>.npy` (float32 [n, 178]: root_orient 3, trans 3,
betas 10, pose_body 63, pose_hand 90, pose_jaw 3, and pose_eye[:, 0:3] TWICE -- the script reads the left eye for both eyes,
preprocessing_amass.py:54-55, and the quirk is kept).

The script runs one full SMPL-X forward per kept frame for one row of 25 joints.  Those joints depend on betas, root_orient,
pose_body and trans only (`hand_pose=` is no argument of `SMPLX.forward`, the hands hang below the wrists, and joints 22..24
are leaves placed by their parent's transform), so joints-only forward kinematics is exact.  Here the host lists, plans, reads
and slices `[::down_sample]`; the frames of many recordings are packed into chunks, and a chunk is one upload per array, one
`rohm_amass_preprocess` launch (float64 -> float32 cast, row assembly, FK) and one copy back per output.

Stated differences from the script: `np.load` runs without `allow_pickle` (the AMASS files need none); a recording with zero
frames is skipped with a message (the script crashes there); a missing key raises an error that names the file; a `BMLrub`
name without a `_` is processed (the script's `split('_')[1]` raises there).
"""
from __future__ import annotations

import argparse
import collections
import concurrent.futures
import glob
import os
import sys
import time

import numpy as np
import torch

EX_FPS = 30                                                      # preprocessing_amass.py:13
FRAME_KEYS = (('root_orient', 3), ('trans', 3), ('pose_body', 63), ('pose_hand', 90), ('pose_jaw', 3), ('pose_eye', 6))
PARAM_COLS, NUM_JOINTS = 178, 25
READER_THREADS = 4                                               # file reads that run ahead of the device (never more than 8)

# the script's argument table (preprocessing_amass.py:146-150): name, type, default, help
SCRIPT_ARGS = (
    ('body_model_path', str, 'data/body_models/smplx_model', 'path to smplx model'),
    ('amass_root', str, '/mnt/hdd/AMASS/AMASS_smplx_neutral', 'Root dir of raw AMASS data (smplx neutral body)'),
    ('dataset_name', str, 'ACCAD', 'AMASS subset name'),
    ('save_root', str, '/mnt/hdd/AMASS/AMASS_smplx_preprocessed', 'Root directory to save preprocessed data to.'),
)
# this package's own arguments
OWN_ARGS = (
    ('device', str, 'cuda:0', 'device that runs the kernel'),
    ('chunk_frames', int, 262144, 'kept frames per launch (a longer recording spans launches)'),
    ('check_against', str, None,
     'DIR: write nothing; compare every file that would be written with the file of the same relative path under DIR (a tree '
     'made by the reference script), print the largest differences and list missing / extra files.  Exit status 0 only if the '
     'file sets agree, the parameter files are bit-equal and the joints are within --check_tol.  No machine this package was '
     'tested on has the smplx package, so the joints of this tool are pinned to the published algorithm only, never to a tree '
     'made by the real package: this option is the pin for machines that have one.'),
    ('check_tol', float, 1e-4, 'largest accepted joint difference in metres for --check_against'),
)


# ---- host: which recordings, which frames -------------------------------------------------------------------------------------
def _scalar(x):
    """A 0-d / one-element array as the Python value the script's comparison sees; anything else unchanged."""
    if isinstance(x, np.ndarray) and x.size == 1:
        return x.reshape(()).item()
    if isinstance(x, np.generic):
        return x.item()
    return x


def _name_rule(dataset_name, recording_name):
    """preprocessing_amass.py:127-134: the reason a recording is skipped by its name, or None."""
    if recording_name == 'neutral_stagei':
        return 'neutral_stagei'
    if dataset_name == 'HDM05' and recording_name[0:12] == 'HDM_dg_07-01':
        return 'HDM05 inline skating'
    if dataset_name == 'BMLrub':
        fields = recording_name.split('_')
        if len(fields) > 1 and fields[1] in ('treadmill', 'normal'):
            return 'BMLrub treadmill'
    return None


def plan_recording(dataset_name, recording_name, fps, gender, surface_model_type):
    """-> (process, down_sample, reason) by the rules of preprocessing_amass.py:23-40 and :127-134.  Values compare as the script
    compares them: a `bytes` gender is unequal to 'neutral'.  `down_sample` is 0 where the recording is skipped by name."""
    rule = _name_rule(dataset_name, recording_name)
    if rule is not None:
        return False, 0, 'skipped by name: ' + rule
    reasons = []
    if _scalar(gender) != 'neutral':
        reasons.append('gender not neutral')
    if _scalar(surface_model_type) != 'smplx':
        reasons.append('not smplx params')
    fps = float(_scalar(fps))
    if dataset_name == 'SSM':                                    # fps = 59.99xx / 120.00xx there
        down_sample = 2 if fps - 60 < 1 else 4
    else:
        down_sample = int(fps / EX_FPS)
        if down_sample != fps / EX_FPS or down_sample < 1:
            reasons.append('frame rate {} not suitable for downsampling to {} fps'.format(fps, EX_FPS))
    return not reasons, down_sample, '; '.join(reasons)


def list_dataset(amass_root, dataset_name):
    """-> (sorted subject directories, sorted [(subject, recording name, path)]) as preprocessing_amass.py:108-125 lists them."""
    base = os.path.join(amass_root, dataset_name)
    subjects = sorted(x for x in os.listdir(base) if os.path.isdir(os.path.join(base, x)))
    paths = sorted(glob.glob(os.path.join(base, '*/*.npz')))
    return subjects, [(p.split('/')[-2], p.split('/')[-1][0:-4], p) for p in paths]


def read_recording(dataset_name, recording_name, path):
    """One raw file -> dict(process, reason, down_sample, frames, betas [10], arrays {key: float64 [n, d]}) with the kept frames
    `[::down_sample]` only."""
    try:
        with np.load(path) as bdata:
            try:
                fps, gender, model = bdata['mocap_frame_rate'], bdata['gender'], bdata['surface_model_type']
                process, ds, reason = plan_recording(dataset_name, recording_name, fps, gender, model)
                out = dict(process=process, reason=reason, down_sample=ds, frames=0)
                if not process:
                    return out
                raw = {k: bdata[k] for k, _ in FRAME_KEYS}
                betas = bdata['betas']
            except KeyError as e:
                raise KeyError(f'{path}: missing key: {e.args[0]}') from None
    except ValueError as e:
        raise ValueError(f'{path}: {e}') from None
    total = raw['trans'].shape[0]
    for k, d in FRAME_KEYS:
        if raw[k].ndim != 2 or raw[k].shape != (total, d):
            raise ValueError(f'{path}: {k} has shape {raw[k].shape}, expected ({total}, {d})')
    if betas.ndim != 1 or betas.shape[0] < 10:
        raise ValueError(f'{path}: betas has shape {betas.shape}, at least 10 values are needed')
    arrays = {k: np.ascontiguousarray(np.asarray(raw[k], np.float64)[::ds]) for k, _ in FRAME_KEYS}
    out.update(frames=len(arrays['trans']), betas=np.asarray(betas[:10], np.float64), arrays=arrays)
    if out['frames'] == 0:
        out.update(process=False, reason='no frames')
    return out


# ---- device ---------------------------------------------------------------------------------------------------------------------
def preprocess_frames(body_model, arrays, betas, rec_of_frame):
    """preprocessing_amass.py:47-69 for the N frames of a chunk in one launch.

    arrays: dict of device float64 tensors 'root_orient' [N,3], 'trans' [N,3], 'pose_body' [N,63], 'pose_hand' [N,90],
    'pose_jaw' [N,3], 'pose_eye' [N,6]; betas [R,10] device float64 (one row per recording); rec_of_frame [N] host integers in
    [0, R), the betas row of each frame.  Returns (joints [N,25,3], params [N,178]) float32 on the device."""
    from ._lib import check, lib, ptr, require_hip, stream_ptr
    from .body_model import native_for
    from .data_loaders.dataloader_amass import _f64
    missing = [k for k, _ in FRAME_KEYS if k not in arrays]
    if missing:
        raise ValueError(f'arrays lacks {missing}')
    require_hip(betas, *[arrays[k] for k, _ in FRAME_KEYS])
    if not torch.is_tensor(betas) or betas.dim() != 2 or betas.shape[1] != 10:
        raise ValueError('betas must be a float64 tensor [R, 10]')
    dev, R = betas.device, int(betas.shape[0])
    N = int(arrays['trans'].shape[0]) if torch.is_tensor(arrays['trans']) and arrays['trans'].dim() == 2 else -1
    if N < 0 or N >= 2 ** 31:
        raise ValueError('trans must be a float64 tensor [N, 3]')
    a = {k: _f64(arrays[k], (N, d), f"arrays['{k}']", dev) for k, d in FRAME_KEYS}
    betas = _f64(betas, (R, 10), 'betas', dev)
    rec = np.asarray(rec_of_frame.cpu() if torch.is_tensor(rec_of_frame) else rec_of_frame)
    if rec.shape != (N,) or rec.dtype.kind not in 'iu':
        raise ValueError(f'rec_of_frame must be {N} integers, got {rec.dtype} {rec.shape}')
    if N and (int(rec.min()) < 0 or int(rec.max()) >= R):
        raise ValueError(f'rec_of_frame must lie in [0, {R}), got [{int(rec.min())}, {int(rec.max())}]')
    nat = native_for(body_model, dev)
    joints = torch.empty(N, NUM_JOINTS, 3, device=dev, dtype=torch.float32)
    params = torch.empty(N, PARAM_COLS, device=dev, dtype=torch.float32)
    rec_dev = torch.from_numpy(np.ascontiguousarray(rec, dtype=np.int32)).to(dev)
    with torch.cuda.device(dev):
        check(lib().rohm_amass_preprocess(nat.handle, *[ptr(a[k]) for k, _ in FRAME_KEYS], ptr(betas), ptr(rec_dev), N, R,
                                          ptr(joints), ptr(params), stream_ptr(dev)), 'rohm_amass_preprocess')
    return joints, params


def _run_chunk(body_model, device, segments):
    """segments: [(recording dict, first kept frame, end)] -> host (joints, params) of the chunk's frames in order."""
    arrays = {k: torch.from_numpy(np.concatenate([r['arrays'][k][a:b] for r, a, b in segments])).to(device) for k, _ in FRAME_KEYS}
    recs, rec_of_frame = [], []
    for r, a, b in segments:
        if not recs or recs[-1] is not r:
            recs.append(r)
        rec_of_frame.append(np.full(b - a, len(recs) - 1, np.int32))
    betas = torch.from_numpy(np.stack([r['betas'] for r in recs])).to(device)
    joints, params = preprocess_frames(body_model, arrays, betas, np.concatenate(rec_of_frame))
    return joints.cpu().numpy(), params.cpu().numpy()


class _Checker:
    """--check_against: compares instead of writing."""

    def __init__(self, root, dataset_name, tol):
        self.root, self.dataset, self.tol = root, dataset_name, tol
        self.seen, self.missing, self.bad = set(), [], []
        self.max_joints = self.max_params = 0.0

    def _one(self, rel, got, bit_equal):
        self.seen.add(rel)
        path = os.path.join(self.root, rel)
        if not os.path.isfile(path):
            self.missing.append(rel)
            return
        ref = np.load(path)
        if ref.shape != got.shape or ref.dtype != got.dtype:
            self.bad.append(f'{rel}: {ref.dtype} {ref.shape} there, {got.dtype} {got.shape} here')
            return
        d = float(np.abs(ref.astype(np.float64) - got.astype(np.float64)).max()) if got.size else 0.0
        d = float('inf') if d != d else d
        if bit_equal:
            self.max_params = max(self.max_params, d)
            if not np.array_equal(ref.view(np.uint32), got.view(np.uint32)):
                self.bad.append(f'{rel}: parameters differ (largest difference {d:.3e})')
        else:
            self.max_joints = max(self.max_joints, d)
            if not d <= self.tol:
                self.bad.append(f'{rel}: joints differ by {d:.3e} m (tolerance {self.tol:.1e})')

    def __call__(self, rel_joints, rel_params, joints, params):
        self._one(rel_joints, joints, False)
        self._one(rel_params, params, True)

    def finish(self, log):
        extra = []
        for tree in ('pose_data_fps_{}'.format(EX_FPS), 'smpl_data_fps_{}'.format(EX_FPS)):
            for p in sorted(glob.glob(os.path.join(self.root, tree, self.dataset, '*/*.npy'))):
                rel = os.path.join(tree, self.dataset, *p.split('/')[-2:])
                if rel not in self.seen:
                    extra.append(rel)
        log(f'[check] {self.dataset}: max |joints difference| {self.max_joints:.3e} m, max |params difference| {self.max_params:.3e}')
        for title, rows in (('missing under ' + self.root, self.missing), ('extra under ' + self.root, extra), ('different', self.bad)):
            for r in rows:
                log(f'[check] {title}: {r}')
        ok = not (self.missing or extra or self.bad)
        return dict(ok=ok, max_joints=self.max_joints, max_params=self.max_params, missing=self.missing, extra=extra,
                    different=self.bad)


def preprocess_dataset(amass_root, dataset_name, save_root, body_model, chunk_frames=262144, log=print, check_against=None,
                       check_tol=1e-4):
    """`main` of preprocessing_amass.py for one AMASS subset.  Returns dict(processed=[relative names], skipped=[(name, reason)],
    frames=kept frames, seconds=dict(read, device, write, wall), chunk_seconds=[upload + kernel + download per chunk]); with
    `check_against` nothing is written and the dict also has 'check' (ok, max_joints, max_params, missing, extra, different)."""
    if int(chunk_frames) < 1:
        raise ValueError('chunk_frames must be at least 1')
    chunk_frames = int(chunk_frames)
    device = body_model.v_template.device
    t_wall = time.perf_counter()
    log('datasets in process: {}'.format(dataset_name))
    subjects, recordings = list_dataset(amass_root, dataset_name)
    trees = ('pose_data_fps_{}'.format(EX_FPS), 'smpl_data_fps_{}'.format(EX_FPS))
    checker = _Checker(check_against, dataset_name, check_tol) if check_against is not None else None
    if checker is None:
        for tree in trees:                                       # every subject gets its folders, also one without a kept recording
            for subj in subjects:
                os.makedirs(os.path.join(save_root, tree, dataset_name, subj), exist_ok=True)
    summary = dict(processed=[], skipped=[], frames=0, seconds=dict(read=0.0, device=0.0, write=0.0, wall=0.0), chunk_seconds=[])
    sec = summary['seconds']

    def timed_read(item):
        t0 = time.perf_counter()
        r = read_recording(dataset_name, item[1], item[2])
        r['read_s'] = time.perf_counter() - t0
        return r

    def emit(item, joints, params):
        t0 = time.perf_counter()
        rel = [os.path.join(tree, dataset_name, item[0], item[1] + '.npy') for tree in trees]
        if checker is not None:
            checker(rel[0], rel[1], joints, params)
        else:
            np.save(os.path.join(save_root, rel[0]), joints)
            np.save(os.path.join(save_root, rel[1]), params)
        sec['write'] += time.perf_counter() - t0
        summary['processed'].append(os.path.join(item[0], item[1]))
        summary['frames'] += len(joints)

    segments, filled, parts = [], 0, {}

    def flush():
        nonlocal segments, filled
        if not segments:
            return
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        joints, params = _run_chunk(body_model, device, segments)
        dt = time.perf_counter() - t0
        sec['device'] += dt
        summary['chunk_seconds'].append(dt)
        at = 0
        for r, a, b in segments:
            got = parts.setdefault(id(r), [])
            got.append((joints[at:at + b - a], params[at:at + b - a]))
            at += b - a
            if b == r['frames']:
                del parts[id(r)]
                one = len(got) == 1
                emit(r['item'], got[0][0] if one else np.concatenate([g[0] for g in got]),
                     got[0][1] if one else np.concatenate([g[1] for g in got]))
        segments, filled = [], 0

    todo = collections.deque()
    for item in recordings:
        rule = _name_rule(dataset_name, item[1])
        if rule is not None:
            summary['skipped'].append((os.path.join(item[0], item[1]), 'skipped by name: ' + rule))
        else:
            todo.append(item)
    with concurrent.futures.ThreadPoolExecutor(max_workers=READER_THREADS) as pool:
        ahead = collections.deque()
        while todo or ahead:
            while todo and len(ahead) < 2 * READER_THREADS:      # a bounded look-ahead: a subset does not fit in memory at once
                item = todo.popleft()
                ahead.append((item, pool.submit(timed_read, item)))
            item, fut = ahead.popleft()
            r = fut.result()
            sec['read'] += r['read_s']
            if not r['process']:
                log('{}: {}'.format(os.path.join(item[0], item[1]), r['reason']))
                summary['skipped'].append((os.path.join(item[0], item[1]), r['reason']))
                continue
            r['item'] = item
            a = 0
            while a < r['frames']:
                b = min(r['frames'], a + chunk_frames - filled)
                segments.append((r, a, b))
                filled += b - a
                a = b
                if filled == chunk_frames:
                    flush()
        flush()
    if checker is not None:
        summary['check'] = checker.finish(log)
    sec['wall'] = time.perf_counter() - t_wall
    log('finished.')
    return summary


# ---- command line ---------------------------------------------------------------------------------------------------------------
def build_parser():
    p = argparse.ArgumentParser(prog='python -m rohm_amd.preprocessing_amass',
                                description='raw AMASS -> pose_data_fps_30 / smpl_data_fps_30 (preprocessing_amass.py) on the device')
    for name, typ, default, text in SCRIPT_ARGS + OWN_ARGS:
        p.add_argument('--' + name, type=typ, default=default, help=text, **({'metavar': 'DIR'} if name == 'check_against' else {}))
    return p


def main(argv=None):
    from .body_model import SMPLXLayer
    from .occlusion import _body_model_file
    args = build_parser().parse_args(argv)
    body = SMPLXLayer.from_npz(_body_model_file(args.body_model_path)).to(torch.device(args.device))
    s = preprocess_dataset(args.amass_root, args.dataset_name, args.save_root, body, chunk_frames=args.chunk_frames,
                           check_against=args.check_against, check_tol=args.check_tol)
    print('[rohm_amd.preprocessing_amass] {}: {} recordings, {} frames, {} skipped; read {:.2f} s, device {:.2f} s, write {:.2f} s'
          .format(args.dataset_name, len(s['processed']), s['frames'], len(s['skipped']), s['seconds']['read'],
                  s['seconds']['device'], s['seconds']['write']))
    return 0 if args.check_against is None or s['check']['ok'] else 1


if __name__ == '__main__':
    sys.exit(main())
