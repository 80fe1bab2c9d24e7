"""How long calibrating a rig takes: the project's ten-minute benchmark track (36 000 frames x 25 joints = 900 000 points) seen by
V = 4 and V = 16 synthetic cameras with distortion and 2 px of noise, through `rohm_amd.rig.pair_hypotheses` (all V (V - 1) / 2
pairs, K = 1024 hypotheses each, one call) and one try of the bundle adjustment (`ba_moments` + `ba_update`), each timed alone with
HIP events around `--inner` back-to-back calls on tensors that are on the device already (median over `--windows` windows after a
warm-up of the same shapes).  Figures: milliseconds per call and Sampson evaluations per second (pairs x hypotheses x points).  The
numpy restatement (tests/rig_ref.py) is timed on the host of the same box on a 70-frame sample with 64 hypotheses, for orientation
only: a restatement written to be read, not a competitor.  Recorded, not judged: the capability is new, nobody has timed another
implementation, no speed-up is claimed.

    python scripts/bench_rig.py [--out profiles/rig_bench.json] [--frames 36000]
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

import rig_ref as RR  # noqa: E402
from bench_multiview import recording  # noqa: E402
from bench_quality import events  # noqa: E402
from rohm_amd import rig  # noqa: E402

DEV = 'cuda:0'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rig_bench.json'))
    ap.add_argument('--frames', type=int, default=36000)
    ap.add_argument('--joints', type=int, default=25)
    ap.add_argument('--views', type=int, nargs='+', default=[4, 16])
    ap.add_argument('--hypotheses', type=int, default=1024)
    ap.add_argument('--host_frames', type=int, default=70)
    ap.add_argument('--host_hypotheses', type=int, default=64)
    ap.add_argument('--inner', type=int, default=1)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--skip_host', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_rig.py measures on the GPU; none found')
    N, J, K = a.frames, a.joints, a.hypotheses
    P = N * J
    res = {'frames': N, 'joints': J, 'points': P, 'hypotheses_per_pair': K, 'inner': a.inner, 'windows': a.windows, 'host_threads': torch.get_num_threads(),
           'note': 'recorded, not judged: no other implementation has been timed and no speed-up is claimed', 'cases': {}}
    for V in a.views:
        kp, cams, _ = recording(V, N, J, 300 + V)
        pairs = np.stack(np.triu_indices(V, 1), 1).astype(np.int32)
        Q = len(pairs)
        g = np.random.Generator(np.random.PCG64(V))
        samples = g.integers(0, P, (Q, K, 8)).astype(np.int32)
        kpd, camd = torch.from_numpy(kp).to(DEV), torch.from_numpy(cams).to(DEV)
        prd, smd = torch.from_numpy(pairs).to(DEV), torch.from_numpy(samples).to(DEV)
        E, counts, best = rig.pair_hypotheses(kpd, camd, prd, smd)
        rows = torch.arange(Q, device=DEV)
        Eb = torch.nan_to_num(E[rows, best.clamp(min=0).long()])
        cnt = counts.cpu().numpy()
        X = torch.from_numpy(np.array([0.0, 0.0, 1.0]) + g.uniform(-0.6, 0.6, (P, 3))).to(DEV)
        dc = torch.zeros(V, 6, device=DEV, dtype=torch.float64)
        c = {'views': V, 'pairs': Q, 'sampson_evaluations_per_call': float(Q) * K * P, 'live_hypotheses': int((cnt[..., 0] >= 0).sum()),
             'median_best_inlier_share': float(np.median(cnt[np.arange(Q), np.maximum(best.cpu().numpy(), 0), 0] / P)),
             'pair_workspace_bytes': rig.pair_ws_bytes(V, P), 'ba_workspace_bytes': rig.ba_ws_bytes(V, P)}
        stages = {'pair_hypotheses': lambda: rig.pair_hypotheses(kpd, camd, prd, smd),
                  'pair_moments': lambda: rig.pair_moments(kpd, camd, prd, Eb),
                  'ba_moments': lambda: rig.ba_moments(kpd, camd, X),
                  'ba_update': lambda: rig.ba_update(kpd, camd, X, dc)}
        for name, fn in stages.items():
            w = events(fn, a.inner, a.windows)
            c[name + '_ms_median'] = round(statistics.median(w), 4)
            c[name + '_ms_min'], c[name + '_ms_max'] = round(min(w), 4), round(max(w), 4)
        c['sampson_evaluations_per_s'] = round(c['sampson_evaluations_per_call'] / (c['pair_hypotheses_ms_median'] * 1e-3), 0)
        c['ba_try_ms'] = round(c['ba_moments_ms_median'] + c['ba_update_ms_median'], 4)
        if not a.skip_host:
            n, k = min(a.host_frames, N), min(a.host_hypotheses, K)
            hs = g.integers(0, n * J, (Q, k, 8)).astype(np.int32)
            t = time.perf_counter()
            ref = RR.pair_hypotheses(kp[:, :n], cams, pairs, hs)
            dt = time.perf_counter() - t
            got = rig.pair_hypotheses(kpd[:, :n].contiguous(), camd, prd, torch.from_numpy(hs).to(DEV))[1].cpu().numpy()
            ok = RR.margins_ok(ref)
            c.update(host_restatement_evaluations=float(Q) * k * n * J, host_restatement_s=round(dt, 4),
                     host_restatement_evaluations_per_s=round(float(Q) * k * n * J / dt, 0),
                     host_restatement_note='tests/rig_ref.py, vectorised numpy: a restatement of the rule, not a competitor; for orientation only',
                     counts_equal_on_the_sample_within_margins=bool(np.array_equal(got[ok], ref['counts'][ok])))
        res['cases']['V%d' % V] = c
        del kpd, smd, E, counts, X
        torch.cuda.empty_cache()
    print(json.dumps(res))
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
