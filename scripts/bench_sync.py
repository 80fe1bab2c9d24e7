"""How long synchronising a rig takes: the project's ten-minute benchmark track (36 000 frames x 25 joints = 900 000 points) seen by
V = 4 and V = 16 synthetic cameras with distortion and 2 px of noise, through `rohm_amd.sync.pair_sweep` -- all V (V - 1) / 2 pairs,
the coarse sweep of a calibrated rig over the integer shifts within +-30 frames (S = 61) and one fine sweep (S = 33, est + k / 16) --
and `rohm_amd.sync.resample_views`, each timed alone with HIP events around `--inner` back-to-back calls on tensors that are on the
device already (median over `--windows` windows after a warm-up of the same shapes).  Figures: milliseconds per call and Sampson
evaluations per second (pairs x shifts x points).  The numpy restatement (tests/sync_ref.py) is timed on the host of the same box on
a 70-frame sample, for orientation only: a restatement written to be read, not a competitor.  Recorded, not judged: the capability
is new, nobody has timed another implementation, no speed-up is claimed.

    python scripts/bench_sync.py [--out profiles/sync_bench.json] [--frames 36000]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import sync_ref as SR  # noqa: E402
from bench_multiview import recording  # noqa: E402
from bench_quality import events  # noqa: E402
from rohm_amd import sync  # noqa: E402

DEV = 'cuda:0'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sync_bench.json'))
    ap.add_argument('--frames', type=int, default=36000)
    ap.add_argument('--joints', type=int, default=25)
    ap.add_argument('--views', type=int, nargs='+', default=[4, 16])
    ap.add_argument('--max_shift', type=int, default=30)
    ap.add_argument('--host_frames', type=int, default=70)
    ap.add_argument('--inner', type=int, default=1)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--skip_host', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_sync.py measures on the GPU; none found')
    N, J, M = a.frames, a.joints, a.max_shift
    P = N * J
    res = {'frames': N, 'joints': J, 'points': P, 'coarse_shifts': 2 * M + 1, 'fine_shifts': 2 * sync.HALF + 1, 'inner': a.inner, 'windows': a.windows,
           'host_threads': torch.get_num_threads(), 'note': 'recorded, not judged: no other implementation has been timed and no speed-up is claimed',
           'cases': {}}
    for V in a.views:
        kp, cams, _ = recording(V, N, J, 300 + V)
        pairs = np.stack(np.triu_indices(V, 1), 1).astype(np.int32)
        Q = len(pairs)
        W = np.broadcast_to(np.eye(4), (V, 4, 4)).copy()
        W[:, :3, :3], W[:, :3, 3] = cams[:, :9].reshape(V, 3, 3), cams[:, 9:12]
        E = np.stack([sync.essential(W, v1, v2) for v1, v2 in pairs])
        g = np.random.Generator(np.random.PCG64(V))
        coarse = np.broadcast_to(np.arange(-M, M + 1, dtype=np.float64), (Q, 2 * M + 1)).copy()
        fine = g.uniform(-M, M, (Q, 1)) + np.arange(-sync.HALF, sync.HALF + 1, dtype=np.float64) / sync.GRID
        kpd, camd, prd, Ed = (torch.from_numpy(x).to(DEV) for x in (kp, cams, pairs, E))
        cd, fd = torch.from_numpy(coarse).to(DEV), torch.from_numpy(fine).to(DEV)
        shv = torch.from_numpy(g.uniform(-M, M, V)).to(DEV)
        out = sync.pair_sweep(kpd, camd, prd, Ed, cd).cpu().numpy()
        c = {'views': V, 'pairs': Q, 'workspace_bytes': sync.ws_bytes(V, P), 'coarse_evaluations_per_call': float(Q) * coarse.shape[1] * P,
             'fine_evaluations_per_call': float(Q) * fine.shape[1] * P, 'median_inlier_share_at_shift_0': float(np.median(out[:, M, 1] / out[:, M, 0])),
             'median_inlier_share_at_other_shifts': float(np.median(np.delete(out[..., 1] / np.maximum(out[..., 0], 1), M, 1)))}
        stages = {'coarse_sweep': lambda: sync.pair_sweep(kpd, camd, prd, Ed, cd), 'fine_sweep': lambda: sync.pair_sweep(kpd, camd, prd, Ed, fd),
                  'resample': lambda: sync.resample_views(kpd, shv)}
        for name, fn in stages.items():
            w = events(fn, a.inner, a.windows)
            c[name + '_ms_median'] = round(statistics.median(w), 4)
            c[name + '_ms_min'], c[name + '_ms_max'] = round(min(w), 4), round(max(w), 4)
        for name in ('coarse', 'fine'):
            c[name + '_evaluations_per_s'] = round(c[name + '_evaluations_per_call'] / (c[name + '_sweep_ms_median'] * 1e-3), 0)
        c['resample_gb_per_s'] = round(24.0 * V * P / (c['resample_ms_median'] * 1e-3) / 1e9, 1)
        if not a.skip_host:
            n = min(a.host_frames, N)
            sh = np.clip(fine, -n + 2, n - 2)
            t = time.perf_counter()
            ref, mt, mi = SR.pair_sweep(kp[:, :n], cams, pairs, E, sh, with_margins=True)
            dt = time.perf_counter() - t
            got = sync.pair_sweep(kpd[:, :n].contiguous(), camd, prd, Ed, torch.from_numpy(sh).to(DEV)).cpu().numpy()
            ok = (mt >= 1e-6) & (mi >= 1e-9)
            c.update(host_restatement_evaluations=float(Q) * sh.shape[1] * n * J, host_restatement_s=round(dt, 4),
                     host_restatement_evaluations_per_s=round(float(Q) * sh.shape[1] * n * J / dt, 0),
                     host_restatement_note='tests/sync_ref.py, vectorised numpy: a restatement of the rule, not a competitor; for orientation only',
                     counts_equal_on_the_sample_within_margins=bool(np.array_equal(got[ok][:, :2], ref[ok][:, :2])))
        res['cases']['V%d' % V] = c
        del kpd, out
        torch.cuda.empty_cache()
    print(json.dumps(res))
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
