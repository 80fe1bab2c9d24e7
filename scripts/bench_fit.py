"""How long fitting SMPL-X to a 3-D skeleton takes: a synthetic 3 000-frame skeleton (a walking synthetic body, 5 mm of noise, 5 %
of the joints unobserved) through the stages of `rohm_amd.fit.fit_joints` -- the first pose pass from the torso triad, a pose pass
from the last solution with smoothing, the shape moments -- each timed alone with HIP events around `--inner` back-to-back calls
on tensors that are on the device already (median over `--windows` windows after a warm-up of the same shapes), the launches per
stage from the library's own profiler, `fit_joints` as a caller with host arrays sees it (a host clock; it reads every pass back),
and the frames per second of the numpy restatement (tests/fit_ref.py) on the host of the same box for a 64-frame sample: a
restatement written to be read, not a competitor.  Recorded, not judged: the capability is new, there is no earlier figure.

    python scripts/bench_fit.py [--out profiles/fit_bench.json] [--frames 3000] [--iters 20]
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

import fit_ref as FR  # noqa: E402
from bench_quality import events, timed  # noqa: E402
from rohm_amd import _lib  # noqa: E402
from rohm_amd import fit as FT  # noqa: E402
from rohm_amd.body_model import SMPLXLayer, native_for  # noqa: E402
from rohm_amd.utils import synth  # noqa: E402

DEV = 'cuda:0'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fit_bench.json'))
    ap.add_argument('--frames', type=int, default=3000)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--host_frames', type=int, default=64)
    ap.add_argument('--inner', type=int, default=3)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--skip_host', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_fit.py measures on the GPU; none found')
    N = a.frames
    tensors = synth.synthetic_smplx_tensors(0)
    layer = SMPLXLayer.from_tensors(tensors).to(DEV)
    nat = native_for(layer, torch.device(DEV))
    joints, _, _, betas = FR.make_frames(tensors, N, seed=7, pose_scale=0.12, beta_scale=0.5, noise=0.005, walk=True)
    g = np.random.Generator(np.random.PCG64(8))
    conf = (g.uniform(size=(N, 22)) >= 0.05).astype(np.float32)
    res = {'frames': N, 'iters': a.iters, 'unobserved_fraction': float(1.0 - conf.mean()), 'inner': a.inner, 'windows': a.windows,
           'fit_pose_registers_and_lds': 'held to 256 VGPRs (25 spilled, 40 B of scratch per lane), 66 472 B of LDS: two workgroups of 4 waves per CU'}
    yd, cd = torch.from_numpy(joints).to(DEV), torch.from_numpy(conf).to(DEV)
    bd = torch.from_numpy(np.repeat(betas[None].astype(np.float32), N, axis=0)).to(DEV)
    wd = torch.from_numpy(FT.default_w_prior()).to(DEV)
    kw = dict(w_prior=wd, iters=a.iters)
    p1, r1, _ = FT.fit_pose(nat, yd, cd, bd, **kw)
    sol = torch.where(r1[:, :1] == 1, p1, torch.full_like(p1, float('nan')))
    use = (r1[:, 0] == 1).to(torch.uint8)
    stages = {'pose_from_triad': lambda: FT.fit_pose(nat, yd, cd, bd, **kw),
              'pose_smoothing_pass': lambda: FT.fit_pose(nat, yd, cd, bd, init=sol, prev=sol, w_smooth=FT.W_SMOOTH, **kw),
              'pose_evaluate_only': lambda: FT.fit_pose(nat, yd, cd, bd, w_prior=wd, iters=0),
              'shape_moments': lambda: FT.shape_moments(nat, yd, cd, p1, use)}
    for name, fn in stages.items():
        w = events(fn, a.inner, a.windows)
        _lib.profile_start()
        fn()
        torch.cuda.synchronize()
        rows = _lib.profile_stop()
        res[name + '_ms_median'] = round(statistics.median(w), 4)
        res[name + '_ms_min'], res[name + '_ms_max'] = round(min(w), 4), round(max(w), 4)
        res[name + '_launches'] = {k: v['launches'] for k, v in rows.items()}
    res['pose_from_triad_frames_per_s'] = round(N / (res['pose_from_triad_ms_median'] * 1e-3), 0)
    r = r1.cpu().numpy()
    ok = r[:, 0] == 1
    res.update(fitted=int(ok.sum()), accepted_iterations_mean=float(r[ok, 3].mean()), residual_median_mm=float(np.median(r[ok, 5]) * 1e3),
               residual_worst_mm=float(r[ok, 5].max() * 1e3))
    w = timed(lambda: FT.fit_joints(joints, conf=conf, betas=betas, iters=a.iters, body_model=layer, device=DEV), 1, a.windows)
    res.update(fit_joints_host_arrays_ms_median=round(statistics.median(w), 3), fit_joints_stages='pass 1, the warm start of the frames without a triad, one smoothing pass')
    if not a.skip_host:
        n = min(a.host_frames, N)
        mdl = FR.model(tensors)
        t = time.perf_counter()
        pw, rw, _ = FR.fit_pose(mdl, joints[:n], conf[:n], np.repeat(betas[None], n, axis=0), w_prior=FT.default_w_prior(), iters=a.iters)
        dt = time.perf_counter() - t
        res.update(host_restatement_frames=n, host_restatement_s=round(dt, 3), host_restatement_frames_per_s=round(n / dt, 2),
                   host_restatement_note='tests/fit_ref.py, numpy, one frame at a time: a restatement of the rule, not a competitor',
                   host_threads=torch.get_num_threads())
        both = ok[:n] & (rw[:, 0] == 1)
        res['energy_end_ratio_vs_restatement_max'] = float((r[:n][both, 2] / rw[both, 2]).max())
    print(json.dumps(res))
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
