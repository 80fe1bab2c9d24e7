"""How long fitting SMPL-X to 2-D keypoints takes: a synthetic 3 000-frame recording (a walking synthetic body, 2 px of noise, 5 %
of the detections unobserved) seen by V = 1, 4 and 16 cameras, through `rohm_fit_views_pose` from a start 0.05 rad off with the
translation solved by the kernel, timed alone with HIP events around `--inner` back-to-back calls on tensors that are on the
device already (median over `--windows` windows after a warm-up of the same shapes), and next to it `rohm_fit_pose` on the 3-D
joints of the same frames: the kernel this one was derived from, at the same N and iterations.  Recorded, not judged: the
capability is new, there is no earlier figure, and no other implementation was timed.

    python scripts/bench_fit_views.py [--out profiles/fit_views_bench.json] [--frames 3000] [--iters 20]

An experiment library (scripts/build_variant.py NAME -DROHM_FIT_VIEWS_ONE_WORKGROUP, selected with ROHM_HIP_LIB) pads the kernel's
LDS past 80 KiB so that one workgroup has a CU to itself: run this script under both and keep both files.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import fit_views_ref as VR  # noqa: E402
from bench_quality import events  # noqa: E402
from rohm_amd import fit as FT  # noqa: E402
from rohm_amd import fit_views as FV  # noqa: E402
from rohm_amd.body_model import SMPLXLayer, native_for  # noqa: E402
from rohm_amd.utils import synth  # noqa: E402

DEV = 'cuda:0'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fit_views_bench.json'))
    ap.add_argument('--frames', type=int, default=3000)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--views', type=int, nargs='+', default=[1, 4, 16])
    ap.add_argument('--inner', type=int, default=3)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--note', default='')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_fit_views.py measures on the GPU; none found')
    N = a.frames
    tensors = synth.synthetic_smplx_tensors(0)
    nat = native_for(SMPLXLayer.from_tensors(tensors).to(DEV), torch.device(DEV))
    res = {'frames': N, 'iters': a.iters, 'inner': a.inner, 'windows': a.windows, 'library': os.path.basename(os.environ.get('ROHM_HIP_LIB', '')) or 'shipped', 'note': a.note,
           'fit_views_pose_registers_and_lds': '255 VGPRs, no spills, 77 848 B of LDS: two workgroups of 4 waves per CU (the one-workgroup '
                                               'experiment library pads the LDS to 86 040 B)'}
    g = np.random.Generator(np.random.PCG64(8))
    for V in a.views:
        cams = VR.make_rig(V, 7 + V, distorted=(0,))
        joints, truth, betas = VR.make_body(tensors, N, 9, root_base=VR.facing(cams), root_angle=0.5, beta_scale=0.5, walk=True)
        kp = VR.make_keypoints(cams, joints, 10 + V, noise_px=2.0)
        kp[..., 2] *= (g.uniform(size=kp.shape[:3]) >= 0.05)
        init = truth.copy()
        init[:, :VR.NROT] += g.standard_normal((N, VR.NROT)) * 0.05
        init[:, VR.NROT:] = np.nan
        kd, cd, idv = (torch.from_numpy(x).to(DEV) for x in (kp, cams, init))
        bd = torch.from_numpy(np.repeat(betas[None].astype(np.float32), N, axis=0)).to(DEV)
        wd = torch.from_numpy(FV.default_w_prior(V)).to(DEV)
        kw = dict(w_prior=wd, sigma_px=FV.SIGMA_PX, iters=a.iters)
        p, r, _, _ = FV.fit_views_pose(nat, kd, cd, bd, idv, **kw)
        sol = torch.where(r[:, :1] == 1, p, torch.full_like(p, float('nan')))
        stages = {'fit': lambda: FV.fit_views_pose(nat, kd, cd, bd, idv, **kw),
                  'smoothing_pass': lambda: FV.fit_views_pose(nat, kd, cd, bd, sol, prev=sol, w_smooth=FV.W_SMOOTH, w_smooth_t=FV.W_SMOOTH_T, **kw),
                  'evaluate_only': lambda: FV.fit_views_pose(nat, kd, cd, bd, idv, w_prior=wd, sigma_px=FV.SIGMA_PX, iters=0)}
        for name, fn in stages.items():
            w = events(fn, a.inner, a.windows)
            key = f'views_{V}_{name}'
            res[key + '_ms_median'] = round(statistics.median(w), 4)
            res[key + '_ms_min'], res[key + '_ms_max'] = round(min(w), 4), round(max(w), 4)
        res[f'views_{V}_fit_us_per_frame'] = round(res[f'views_{V}_fit_ms_median'] * 1e3 / N, 3)
        rh = r.cpu().numpy()
        ok = rh[:, 0] == 1
        res[f'views_{V}_fitted'] = int(ok.sum())
        res[f'views_{V}_accepted_iterations_mean'] = float(rh[ok, 3].mean())
        res[f'views_{V}_reprojection_rms_median_px'] = float(np.median(rh[ok, 5]))
        if V == a.views[0]:                          # rohm_fit_pose on the 3-D joints of the same frames, the same N and iterations
            yd = torch.from_numpy(joints.astype(np.float32)).to(DEV)
            w3 = torch.from_numpy(FT.default_w_prior()).to(DEV)
            w = events(lambda: FT.fit_pose(nat, yd, None, bd, w_prior=w3, iters=a.iters), a.inner, a.windows)
            res['fit_pose_3d_ms_median'] = round(statistics.median(w), 4)
            res['fit_pose_3d_us_per_frame'] = round(res['fit_pose_3d_ms_median'] * 1e3 / N, 3)
    print(json.dumps(res))
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
