"""How long the native AMASS loader takes to build a training set and to hand out a batch: `DataloaderAMASS` (split 'train',
task 'pose', parameter noise at the stage-1 stds) on a synthetic tree of `--clips` clips of `--clip_len` frames (default 64
clips of 145) and one `batches(--batch)` batch of it, against the numpy / scipy restatement of the reference's loader
(tests/amass_ref.py + oracle/; kind "port", as bench.py names a host baseline made of the oracle) on the host of the same box.

Device: the constructor is wall clock around a synchronised call (it reads the files, draws the noise on the host and runs
every launch), median over `--windows` calls after a warm-up; the batch is HIP events around `--inner` back-to-back batches,
median over `--windows` windows.  Host: wall clock of one construction and of collating `--batch` items.  The restatement
runs the body model once per clip, like the reference.  Recorded, not judged.

    python scripts/bench_amass_loader.py [--out profiles/amass_loader_timing.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import amass_ref as AR  # noqa: E402
from oracle import geometry as G  # noqa: E402
from rohm_amd.body_model import SMPLXLayer  # noqa: E402
from rohm_amd.data_loaders.dataloader_amass import DataloaderAMASS  # noqa: E402
from rohm_amd.utils import synth  # noqa: E402

DEV = 'cuda:0'


def write_tree(root, n_clips, clip_len, per_seq=8):
    """`n_clips` clips in sequences of `per_seq` clips (+ 7 frames that `divide_clip` drops)."""
    arrays, left, k = {}, n_clips, 0
    while left > 0:
        c = min(per_seq, left)
        jw, world = synth.synthetic_recording(100 + k, c * clip_len + 7, 'z')
        joints, smplx = np.zeros((len(jw), 25, 3), np.float32), np.zeros((len(jw), 178))
        joints[:, :22], smplx[:, :79] = jw, world
        arrays[f'Synth/seq{k:03d}'] = (joints, smplx)
        left, k = left - c, k + 1
    return AR.write_tree(root, arrays)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'amass_loader_timing.json'))
    ap.add_argument('--clips', type=int, default=64)
    ap.add_argument('--clip_len', type=int, default=145)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--inner', type=int, default=50)
    ap.add_argument('--windows', type=int, default=9)
    ap.add_argument('--skip_host', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_amass_loader.py measures on the GPU; none found')
    tensors = synth.synthetic_smplx_tensors(0)
    layer = SMPLXLayer.from_tensors(tensors).to(DEV)
    with tempfile.TemporaryDirectory() as tmp:
        root, logdir = write_tree(os.path.join(tmp, 'amass'), a.clips, a.clip_len), os.path.join(tmp, 'log')
        kw = dict(split='train', task='pose', input_noise=True, clip_len=a.clip_len, **AR.STAGE1_STD)

        def construct():
            np.random.seed(0)
            t = time.perf_counter()
            ds = DataloaderAMASS(preprocessed_amass_root=root, body_model_path=layer, amass_datasets=['Synth'], logdir=logdir,
                                 device=DEV, **kw)
            torch.cuda.synchronize()
            return ds, time.perf_counter() - t

        for _ in range(2):
            ds, _ = construct()
        build = [construct()[1] * 1e3 for _ in range(a.windows)]
        for _ in range(3):
            batch = next(iter(ds.batches(a.batch)))
        torch.cuda.synchronize()
        times = []
        for _ in range(a.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                next(iter(ds.batches(a.batch)))
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) / a.inner)
        res = {'clips': ds.n_samples, 'clip_len': a.clip_len, 'batch': int(batch['motion_repr_clean'].shape[0]),
               'windows': a.windows, 'inner_batches': a.inner,
               'device_build_ms_median': round(statistics.median(build), 3), 'device_build_ms_min': round(min(build), 3),
               'device_build_ms_max': round(max(build), 3), 'device_batch_ms_median': round(statistics.median(times), 4),
               'device_batch_ms_min': round(min(times), 4), 'device_batch_ms_max': round(max(times), 4)}
        if not a.skip_host:
            body = G.BodyModel(tensors)
            np.random.seed(0)
            t = time.perf_counter()
            ref = AR.Loader(root, body, ['Synth'], **kw)
            t_build = time.perf_counter() - t
            items = [ref[i] for i in range(min(a.batch, len(ref)))]
            host_batch = {k: np.stack([it[k] for it in items]) for k in items[0]}
            t_batch = time.perf_counter() - t - t_build
            dev_noisy = ds._device_data['noisy'].cpu().numpy()
            res['host'] = {'kind': 'port', 'build_s': round(t_build, 3), 'batch_s': round(t_batch, 4),
                           'threads': torch.get_num_threads(), 'host_cpus': os.cpu_count()}
            res['max_abs_diff_repr_clean'] = float(np.abs(ds._device_data['clean'].cpu().numpy() - ref.repr_clean).max())
            res['max_abs_diff_repr_noisy_without_contact'] = float(np.abs(dev_noisy - np.asarray(ref.repr_noisy))[..., :290].max())
            res['batch_shape'] = list(host_batch['motion_repr_noisy'].shape)
    print(json.dumps(res))
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
