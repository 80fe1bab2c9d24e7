"""How long triangulating a recording takes: the project's ten-minute benchmark track (36 000 frames x 25 joints = 900 000 points)
seen by V = 4 and V = 16 synthetic cameras with distortion, 2 px of noise and one mis-detection per point, through
`rohm_amd.multiview.triangulate` (one launch) and `view_residuals`, each timed alone with HIP events around `--inner`
back-to-back calls on tensors that are on the device already (median over `--windows` windows after a warm-up of the same shapes).
Figures: milliseconds per call, points and pair evaluations per second (every pair of observed views counts once, scored or
skipped).  For comparison: the time the keypoints alone take to stream from HBM at the 6.29 TB/s a float4 copy reaches on this
chip (the floor a memory-bound form of the kernel could reach), and a measured device copy of them (read + write).  The
vectorised numpy restatement (tests/multiview_ref.py) is timed on the host of the same box on a 70-frame sample: a restatement
written to be read, not a competitor.  Recorded, not judged: the capability is new, nobody has timed another implementation,
no speed-up is claimed.

    python scripts/bench_multiview.py [--out profiles/multiview_bench.json] [--frames 36000]
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

import multiview_ref as MR  # noqa: E402
from bench_quality import events  # noqa: E402
from rohm_amd import _lib  # noqa: E402
from rohm_amd import multiview as MV  # noqa: E402

DEV = 'cuda:0'
HBM_COPY_BYTES_PER_S = 6.29e12      # measured float4 copy on the MI355X (8.0 TB/s spec)


def recording(V, N, J, seed):
    """-> (keypoints [V,N,J,3] float32, cams [V,24], rigid [12]): points about the rig's centre, 2 px of noise, and in one view per
    point a detection 60 .. 300 px off."""
    K, W, D = MR.make_rig(V, seed, True)
    cams = MV.pack_cameras(K, W, D)
    g = np.random.Generator(np.random.PCG64(seed + 1))
    kp = np.empty((V, N * J, 3), np.float32)
    step = 90000
    for s in range(0, N * J, step):                  # in slices: 16 views x 900 000 points of float64 temporaries are large
        n = min(step, N * J - s)
        X = np.array([0.0, 0.0, 1.0]) + g.uniform(-0.6, 0.6, (n, 3))
        px, _ = MR.project(cams, X)
        px += g.standard_normal(px.shape) * 2.0
        bad, ang, rad = g.integers(0, V, n), g.uniform(0, 2 * np.pi, n), g.uniform(60.0, 300.0, n)
        px[bad, np.arange(n)] += np.stack([rad * np.cos(ang), rad * np.sin(ang)], -1)
        kp[:, s:s + n, :2] = px
        kp[:, s:s + n, 2] = g.uniform(0.5, 1.0, (V, n))
    return kp.reshape(V, N, J, 3), cams, np.concatenate([W[0, :3, :3].reshape(9), W[0, :3, 3]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'multiview_bench.json'))
    ap.add_argument('--frames', type=int, default=36000)
    ap.add_argument('--joints', type=int, default=25)
    ap.add_argument('--views', type=int, nargs='+', default=[4, 16])
    ap.add_argument('--host_frames', type=int, default=70)
    ap.add_argument('--inner', type=int, default=5)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--skip_host', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_multiview.py measures on the GPU; none found')
    N, J = a.frames, a.joints
    res = {'frames': N, 'joints': J, 'points': N * J, 'inner': a.inner, 'windows': a.windows, 'host_threads': torch.get_num_threads(),
           'kernel_registers_and_lds': ('16 lanes per point up to V = 6: 108 VGPRs, 6 912 B of LDS per workgroup of 16 points; a wave per point above: 106 VGPRs, '
                                        '4 608 B per workgroup of 4 points; no scratch'), 'cases': {}}
    for V in a.views:
        kp, cams, rigid = recording(V, N, J, 300 + V)
        kpd, camd, rgd = torch.from_numpy(kp).to(DEV), torch.from_numpy(cams).to(DEV), torch.from_numpy(rigid).to(DEV)
        tri = MV.triangulate(kpd, camd, rigid=rgd, want_undistorted=True)
        world = MV.triangulate(kpd, camd).joints
        report = tri.report.cpu().numpy()
        n_obs = report[..., 3]
        pairs = float((n_obs * (n_obs - 1) / 2).sum())
        c = {'views': V, 'keypoint_bytes': int(kp.nbytes), 'pairs_per_call': pairs,
             'points_with_a_result': int((report[..., 0] > 0).sum()), 'median_inliers': float(np.median(report[..., 0])),
             'median_sigma_m': float(np.nanmedian(report[..., 2])), 'median_rms_px': float(np.nanmedian(report[..., 1]))}
        stages = {'triangulate': lambda: MV.triangulate(kpd, camd),
                  'triangulate_rigid_and_undistorted': lambda: MV.triangulate(kpd, camd, rigid=rgd, want_undistorted=True),
                  'triangulate_no_refinement': lambda: MV.triangulate(kpd, camd, refine=0),
                  'view_residuals': lambda: MV.view_residuals(world, kpd, camd),
                  'device_copy_of_the_keypoints': lambda: kpd.clone()}
        for name, fn in stages.items():
            w = events(fn, a.inner, a.windows)
            c[name + '_ms_median'] = round(statistics.median(w), 4)
            c[name + '_ms_min'], c[name + '_ms_max'] = round(min(w), 4), round(max(w), 4)
        _lib.profile_start()
        stages['triangulate']()
        torch.cuda.synchronize()
        c['triangulate_launches'] = {k: v['launches'] for k, v in _lib.profile_stop().items()}
        ms = c['triangulate_ms_median']
        c['points_per_s'] = round(N * J / (ms * 1e-3), 0)
        c['pair_evaluations_per_s'] = round(pairs / (ms * 1e-3), 0)
        c['hbm_floor_ms_keypoints_at_6p29_TB_per_s'] = round(kp.nbytes / HBM_COPY_BYTES_PER_S * 1e3, 4)
        c['times_the_hbm_floor'] = round(ms / c['hbm_floor_ms_keypoints_at_6p29_TB_per_s'], 1)
        if not a.skip_host:
            n = min(a.host_frames, N)
            MR.triangulate(kp[:, :3], cams)
            t = time.perf_counter()
            ref = MR.triangulate(kp[:, :n], cams)
            dt = time.perf_counter() - t
            got = tri.report.cpu().numpy()[:n]
            c.update(host_restatement_points=n * J, host_restatement_s=round(dt, 4), host_restatement_points_per_s=round(n * J / dt, 0),
                     host_restatement_note='tests/multiview_ref.py, vectorised numpy: a restatement of the rule, not a competitor',
                     inlier_counts_equal_on_the_sample=bool(np.array_equal(got[..., 0], ref['report'][..., 0])))
        res['cases']['V%d' % V] = c
        del kpd, tri, world
        torch.cuda.empty_cache()
    print(json.dumps(res))
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
