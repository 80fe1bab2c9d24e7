"""How long a generic track takes to get ready: `resample_track` (one launch of `rohm_track_resample` plus its uploads and the
read-back of the valid list) and the whole `DataloaderTrack` build, for a synthetic ten-minute 60 fps track with detector
holes (36 000 source frames -> 18 000 frames at 30 fps, clips of 145 with overlap 2), against the numpy restatement of the
resampling rule (tests/track_ref.py) on the host of the same box.

Device-side times: a host clock around calls that end in a device synchronise, median over `--windows` windows of `--inner`
calls after a warm-up of the same shapes; the kernel alone with HIP events around `--inner` back-to-back launches on tensors
that are on the device already.  Host time: wall clock of one pass.  Recorded, not judged: nobody runs this path in a loop.

    python scripts/bench_track.py [--out profiles/track_bench.json] [--minutes 10] [--fps 60]
"""
import argparse
import json
import os
import pickle
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import track_ref as TR  # noqa: E402
import video_tree as VT  # noqa: E402
from rohm_amd.body_model import SMPLXLayer  # noqa: E402
from rohm_amd.data_loaders.track import DataloaderTrack, default_max_gap, plan_times, read_track, resample_track  # noqa: E402
from rohm_amd.utils import synth  # noqa: E402

DEV = 'cuda:0'


def synthetic_track(n, fps, seed=0):
    """World motion of `video_tree.tree_motion` is 30 fps; here: smooth rotations (|angle| < 1.5 rad) and a slow drift, holes of
    1 .. 12 frames over about 3 % of the frames."""
    g = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n) / fps
    f, ph = g.uniform(0.05, 0.4, size=79), g.uniform(0, 2 * np.pi, size=79)
    p = 0.45 * np.sin(2 * np.pi * f * t[:, None] + ph)
    p[:, 3:6] = p[:, 3:6] + np.array([0.0, 0.0, 3.0])
    p[:, 6:16] = g.standard_normal(10) * 0.3
    p[:, 0:3] += np.array([np.pi / 2, 0.0, 0.0]) * 0.9                   # upright in a y-down camera, roughly
    valid = np.ones(n, bool)
    for s in g.integers(1, n - 13, size=n // 200):
        valid[s:s + int(g.integers(1, 13))] = False
    kp = np.concatenate([g.uniform(size=(n, 25, 2)) * np.array([1920.0, 1080.0]), g.uniform(size=(n, 25, 1))], -1).astype(np.float32)
    cam2world = np.eye(4)
    cam2world[:3, :3] = np.array([[1.0, 0, 0], [0, 0, 1.0], [0, -1.0, 0]])
    return {'global_orient': p[:, 0:3].astype(np.float32), 'transl': p[:, 3:6].astype(np.float32), 'betas': p[0, 6:16].astype(np.float32),
            'body_pose': p[:, 16:79].astype(np.float32), 'cam2world': cam2world, 'fps': float(fps), 'valid': valid, 'keypoints_2d': kp,
            'mask_joint': (g.uniform(size=(n, 25)) > 0.3).astype(np.float32), 'focal_length': np.array([1060.0, 1060.0]),
            'camera_center': np.array([960.0, 540.0]), 'floor_height': 0.0}


def timed(fn, inner, windows):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        t = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) / inner * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'track_bench.json'))
    ap.add_argument('--minutes', type=float, default=10.0)
    ap.add_argument('--fps', type=float, default=60.0)
    ap.add_argument('--clip_len', type=int, default=145)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--skip_host', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_track.py measures on the GPU; none found')
    n = int(round(a.minutes * 60 * a.fps))
    rec = read_track(synthetic_track(n, a.fps))
    ts, valid, p79, kp, mask = rec['times'], rec['valid'], rec['params79'], rec['keypoints'], rec['mask_joint']
    td = plan_times(ts, valid)
    max_gap = default_max_gap(ts)
    res = {'source_frames': n, 'source_fps': a.fps, 'valid_frames': int(valid.sum()), 'frames_30fps': len(td), 'clip_len': a.clip_len,
           'inner': a.inner, 'windows': a.windows}

    # the wrapper as a caller sees it: host arrays in, device tensors out
    w = timed(lambda: resample_track(ts, valid, p79, kp, mask, td, max_gap, DEV), a.inner, a.windows)
    res.update(resample_track_ms_median=round(statistics.median(w), 4), resample_track_ms_min=round(min(w), 4),
               resample_track_ms_max=round(max(w), 4))
    # ... and with the big arrays on the device already
    dp, dk, dm = (torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in (p79, kp, mask))
    w = timed(lambda: resample_track(ts, valid, dp, dk, dm, td, max_gap, DEV), a.inner, a.windows)
    res.update(resample_track_device_inputs_ms_median=round(statistics.median(w), 4))
    out = resample_track(ts, valid, dp, dk, dm, td, max_gap, DEV)
    res['gap_frames_30fps'] = int(out['gap'].sum())

    # the whole loader: resample + frames_to_world + build_clips + visibility_masks + one device -> host copy of the items
    tensors = synth.synthetic_smplx_tensors(0)
    layer = SMPLXLayer.from_tensors(tensors).to(DEV)
    with tempfile.TemporaryDirectory() as logdir:
        mean, std = synth.synthetic_stats(5)
        for name, vec in (('AMASS_mean.pkl', mean), ('AMASS_std.pkl', std)):
            with open(os.path.join(logdir, name), 'wb') as f:
                pickle.dump(VT._stats_dict(vec), f)
        build = lambda: DataloaderTrack(rec, body_model_path=layer, logdir=logdir, task='pose', clip_len=a.clip_len, overlap_len=2,  # noqa: E731
                                        use_scene_floor_height=False, device=DEV)
        ds = build()
        w = timed(build, 3, a.windows)
    res.update(loader_clips=len(ds), loader_build_ms_median=round(statistics.median(w), 3), loader_build_ms_min=round(min(w), 3),
               loader_build_ms_max=round(max(w), 3))

    if not a.skip_host:
        t = time.perf_counter()
        ref = TR.resample(ts, valid, p79, kp, mask, td, max_gap)
        res['host_restatement_s'] = round(time.perf_counter() - t, 4)
        res['host_threads'] = torch.get_num_threads()
        got = out['params'].cpu().numpy()
        res['max_geodesic_vs_restatement_rad'] = float(max(TR.geodesic(got[:, c:c + 3], ref['params'][:, c:c + 3]).max() for c in TR.ROT_COLS))
        res['gap_equal'] = bool(np.array_equal(out['gap'].cpu().numpy(), ref['gap']))
    print(json.dumps(res))
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
