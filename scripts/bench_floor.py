"""How long finding the floor of an uncalibrated track takes: `estimate_floor` (csrc/floor.hip: candidates, K = 4096 hypotheses
in one launch, three moment passes, plus the compaction, the uploads and the read-backs in between) from host arrays and with
the arrays on the device, the three entry points alone, and the numpy restatement (tests/floor_ref.py) on the host of the same
box, for the synthetic ten-minute 60 fps track of scripts/bench_track.py (36 000 frames with detector holes; its joints come
from `rohm_smplx_joints`).  That track wanders without a floor, so few of its toes rest: the estimator runs on what it finds
(strict=False), and the kernels are also timed alone at the intended size, `--points` synthetic contacts near a plane.

Device-side times: a host clock around calls that end in a device synchronise (`estimate_floor` reads the best plane and the
moments back), median over `--windows` windows of `--inner` calls after a warm-up of the same shapes; the entry points alone
with HIP events around `--inner` back-to-back calls on tensors that are on the device already.  Host time: wall clock of one
pass of the restatement at `--host_hypotheses` planes (it holds K x NJ distances in memory by chunks).  Recorded, not judged:
nobody has timed another implementation of this path.

    python scripts/bench_floor.py [--out profiles/floor_bench.json] [--minutes 10] [--fps 60] [--hypotheses 4096]
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

import floor_ref as FR  # noqa: E402
from bench_quality import events, timed  # noqa: E402
from bench_track import synthetic_track  # noqa: E402
from rohm_amd import _lib  # noqa: E402
from rohm_amd import floor as FL  # noqa: E402
from rohm_amd.body_model import SMPLXLayer  # noqa: E402
from rohm_amd.utils import synth  # noqa: E402

DEV = 'cuda:0'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'floor_bench.json'))
    ap.add_argument('--minutes', type=float, default=10.0)
    ap.add_argument('--fps', type=float, default=60.0)
    ap.add_argument('--hypotheses', type=int, default=4096)
    ap.add_argument('--points', type=int, default=40000, help='contacts of the kernels-alone timing')
    ap.add_argument('--host_hypotheses', type=int, default=256)
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--skip_host', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_floor.py measures on the GPU; none found')
    n = int(round(a.minutes * 60 * a.fps))
    layer = SMPLXLayer.from_tensors(synth.synthetic_smplx_tensors(0)).to(DEV)
    _, rec, joints = FL.track_joints(synthetic_track(n, a.fps), layer, DEV)
    times, valid, K = rec['times'], rec['valid'], a.hypotheses
    res = {'source_frames': n, 'source_fps': a.fps, 'valid_frames': int(valid.sum()), 'joints': 22 * int(valid.sum()), 'hypotheses': K,
           'inner': a.inner, 'windows': a.windows}
    kw = dict(times=times, valid=valid, hypotheses=K, seed=0, strict=False)
    jh = joints.cpu().numpy()
    try:
        est = FL.estimate_floor(joints, **kw)
    except ValueError as e:                                                          # fewer than three resting toes in this track
        est = None
        res['track_note'] = str(e)
    if est is not None:
        res.update(track_candidates=est.candidates, track_support=est.support, track_under=est.under)
        # as a caller with host arrays sees it: the upload of the joints, the launches, the read-backs
        w = timed(lambda: FL.estimate_floor(torch.from_numpy(jh).to(DEV), **kw), a.inner, a.windows)
        res.update(estimate_floor_host_arrays_ms_median=round(statistics.median(w), 4), estimate_floor_host_arrays_ms_min=round(min(w), 4),
                   estimate_floor_host_arrays_ms_max=round(max(w), 4))
        # ... and with the joints on the device already (`calibrate_track`: they come from rohm_smplx_joints)
        w = timed(lambda: FL.estimate_floor(joints, **kw), a.inner, a.windows)
        res.update(estimate_floor_device_arrays_ms_median=round(statistics.median(w), 4), estimate_floor_device_arrays_ms_min=round(min(w), 4),
                   estimate_floor_device_arrays_ms_max=round(max(w), 4))

    # the three entry points alone, at the intended size
    lib, stream = _lib.lib(), _lib.stream_ptr(torch.device(DEV))
    N, vi = int(joints.shape[0]), torch.from_numpy(np.flatnonzero(valid).astype(np.int32)).to(DEV)
    t_dev, flags = torch.from_numpy(times).to(DEV), torch.empty(N, 2, device=DEV, dtype=torch.uint8)
    cand = lambda: lib.rohm_floor_candidates(joints.data_ptr(), t_dev.data_ptr(), vi.data_ptr(), None, N, int(vi.shape[0]), 0.2, 0.10,  # noqa: E731
                                             FL.default_max_gap(times), flags.data_ptr(), stream)
    assert cand() == 0
    w = events(cand, a.inner, a.windows)
    res['candidates_kernels_ms_median'] = round(statistics.median(w), 5)
    g = np.random.Generator(np.random.PCG64(1))
    P = a.points
    xy = g.uniform(-3.0, 3.0, size=(P, 2))
    pts = np.concatenate([xy, (0.1 * xy[:, :1] + 3.0 + np.where(g.uniform(size=(P, 1)) < 0.2, 0.4, 0.0) + g.normal(0, 0.005, size=(P, 1)))], axis=1)
    pts = torch.from_numpy(pts.astype(np.float32)).to(DEV)
    body = joints.index_select(0, vi.long()).reshape(-1, 3).contiguous()
    NJ = int(body.shape[0])
    tr = torch.from_numpy(FL.draw_triples(P, K, 0)).to(DEV)
    planes, scores = torch.empty(K, 4, device=DEV, dtype=torch.float64), torch.empty(K, 3, device=DEV, dtype=torch.int64)
    best = torch.empty(1, device=DEV, dtype=torch.int32)
    hyp = lambda: lib.rohm_floor_hypotheses(pts.data_ptr(), P, body.data_ptr(), NJ, tr.data_ptr(), K, 0.03, 0.08, planes.data_ptr(),  # noqa: E731
                                            scores.data_ptr(), best.data_ptr(), stream)
    assert hyp() == 0
    w = events(hyp, a.inner, a.windows)
    evals = float(K) * (P + NJ)
    res.update(kernel_points=P, kernel_joints=NJ, hypotheses_kernels_ms_median=round(statistics.median(w), 4), hypotheses_kernels_ms_min=round(min(w), 4),
               hypotheses_kernels_ms_max=round(max(w), 4), plane_evaluations=evals,
               plane_evaluations_per_s=round(evals / (statistics.median(w) * 1e-3), 0))
    h = int(best.cpu()[0])
    plane, origin, out = planes[h].contiguous(), pts[:3].double().mean(dim=0).contiguous(), torch.empty(11, device=DEV, dtype=torch.float64)
    mom = lambda: lib.rohm_floor_moments(pts.data_ptr(), P, plane.data_ptr(), origin.data_ptr(), 0.03, out.data_ptr(), stream)  # noqa: E731
    assert mom() == 0
    w = events(mom, a.inner, a.windows)
    res.update(moments_kernels_ms_median=round(statistics.median(w), 5), kernel_support=int(out.cpu()[0]))

    if not a.skip_host and est is not None:
        kh = dict(kw, hypotheses=a.host_hypotheses)
        t = time.perf_counter()
        ref = FR.estimate_floor(jh, **kh)
        res.update(host_restatement_s=round(time.perf_counter() - t, 4), host_restatement_hypotheses=a.host_hypotheses,
                   host_threads=torch.get_num_threads())
        got = FL.estimate_floor(joints, **kh)
        res['plane_max_abs_vs_restatement'] = float(max(np.abs(got.normal - ref.normal).max(), abs(got.offset - ref.offset)))
        res['counts_equal'] = bool((got.candidates, got.support, got.under, got.hypothesis) == (ref.candidates, ref.support, ref.under, ref.hypothesis))
    print(json.dumps(res))
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
