"""Where the time of `rohm_amd.preprocessing_amass` goes: host reads, upload + kernel + download, writes.

Builds a synthetic raw tree (recordings of realistic lengths at 120 fps, seeded) in a temporary directory -- on a tmpfs when
/dev/shm is there, so that the figures are the tool's and not a disk's -- and runs `preprocess_dataset` over it `--windows` times
after one warm-up run.  Per window it records the seconds the reader threads spent in `np.load` + slicing (summed over the
threads, which overlap the device), the seconds of the chunks (upload + launch + copy back, each between device synchronisations),
the seconds in `np.save`, and the wall clock; the kernel alone is timed with device events on one resident chunk.  Recorded, not
judged: the reference script needs the smplx package and cannot run where this is measured, so no speed-up is stated.

    python scripts/bench_preprocess.py [--out profiles/preprocess_bench.json] [--recordings 240] [--windows 5]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rohm_amd import preprocessing_amass as P  # noqa: E402
from rohm_amd.body_model import SMPLXLayer  # noqa: E402
from rohm_amd.utils import synth  # noqa: E402

DEV = 'cuda:0'
BYTES_PER_FRAME = 8 * 168 + 4 + 4 * (P.PARAM_COLS + P.NUM_JOINTS * 3)      # six float64 inputs, the index, the two float32 outputs


def build_tree(root, recordings, seed):
    """`recordings` files under <root>/ACCAD/<subject>/: 120 fps, log-normal lengths (median 10 s, 2 s .. 60 s)."""
    g = np.random.Generator(np.random.PCG64(seed))
    frames = np.clip(np.exp(g.normal(np.log(1200.0), 0.7, recordings)), 240, 7200).astype(np.int64)
    for i, n in enumerate(frames):
        d = os.path.join(root, 'ACCAD', f's{i // 12:02d}')
        os.makedirs(d, exist_ok=True)
        walk = lambda cols, s: np.cumsum(g.standard_normal((n, cols)) * s, axis=0)
        np.savez(os.path.join(d, f'r{i:03d}_stageii.npz'), mocap_frame_rate=np.array(120.0), gender=np.array('neutral'),
                 surface_model_type=np.array('smplx'), betas=g.standard_normal(16), trans=walk(3, 0.01) + [0.0, 0.0, 1.0],
                 root_orient=walk(3, 0.01), pose_body=walk(63, 0.005), pose_hand=walk(90, 0.002), pose_jaw=walk(3, 0.001),
                 pose_eye=walk(6, 0.001))
    return int(frames.sum())


def spread(xs):
    xs = sorted(xs)
    return dict(median=round(xs[len(xs) // 2], 4), min=round(xs[0], 4), max=round(xs[-1], 4))


def kernel_ms(body, frames, launches):
    g = torch.Generator(device=DEV).manual_seed(0)
    arrays = {k: torch.randn(frames, d, device=DEV, dtype=torch.float64, generator=g) * 0.3 for k, d in P.FRAME_KEYS}
    recs = max(1, frames // 300)
    betas = torch.randn(recs, 10, device=DEV, dtype=torch.float64, generator=g)
    rec = (np.arange(frames) * recs // frames).astype(np.int32)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    P.preprocess_frames(body, arrays, betas, rec)                           # warm-up: code object, allocator
    torch.cuda.synchronize()
    for a, b in ev:                                                         # the events bracket the index upload and the launch
        a.record()
        P.preprocess_frames(body, arrays, betas, rec)
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'preprocess_bench.json'))
    ap.add_argument('--recordings', type=int, default=240)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--chunk_frames', type=int, default=262144)
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_preprocess needs the GPU: nothing is measured without one')
    body = SMPLXLayer.from_tensors(synth.synthetic_smplx_tensors(0)).to(DEV)
    base = tempfile.mkdtemp(prefix='rohm_preprocess_', dir='/dev/shm' if os.path.isdir('/dev/shm') and os.access('/dev/shm', os.W_OK) else None)
    try:
        t0 = time.perf_counter()
        raw_frames = build_tree(os.path.join(base, 'raw'), args.recordings, args.seed)
        res = {'device': torch.cuda.get_device_name(0), 'recordings': args.recordings, 'raw_frames': raw_frames, 'fps': 120,
               'chunk_frames': args.chunk_frames, 'reader_threads': P.READER_THREADS, 'windows': args.windows,
               'tree_on': 'tmpfs' if base.startswith('/dev/shm') else 'temporary directory',
               'tree_build_s': round(time.perf_counter() - t0, 2)}
        runs = []
        for w in range(args.windows + 1):                                   # window 0 is the warm-up
            out = os.path.join(base, 'out')
            shutil.rmtree(out, ignore_errors=True)
            s = P.preprocess_dataset(os.path.join(base, 'raw'), 'ACCAD', out, body, chunk_frames=args.chunk_frames, log=lambda *_: None)
            if w:
                runs.append(s)
        res['kept_frames'] = runs[0]['frames']
        res['chunks_per_run'] = len(runs[0]['chunk_seconds'])
        res['host_read_s'] = spread([r['seconds']['read'] for r in runs])
        res['upload_kernel_download_s'] = spread([r['seconds']['device'] for r in runs])
        res['write_s'] = spread([r['seconds']['write'] for r in runs])
        res['wall_s'] = spread([r['seconds']['wall'] for r in runs])
        res['kept_frames_per_wall_s'] = round(res['kept_frames'] / res['wall_s']['median'], 1)
        n = min(args.chunk_frames, res['kept_frames'])
        ms = kernel_ms(body, n, 20)
        res['kernel_frames'] = n
        res['index_upload_and_kernel_ms'] = spread(ms)
        res['kernel_gbytes_per_s_algorithmic'] = round(BYTES_PER_FRAME * n / (res['index_upload_and_kernel_ms']['median'] * 1e-3) / 1e9, 1)
        res['note'] = ('host_read_s is summed over the reader threads and overlaps the device; the reference script was not run '
                       '(it needs the smplx package), so no speed-up is stated')
    finally:
        shutil.rmtree(base, ignore_errors=True)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
