"""How long the clip side of a PROX recording takes: `frames_to_world` + `build_clips` + `visibility_masks` on the device
against the numpy / scipy restatement of the same work (tests/clips_ref.py + oracle/) on the host of the same box, for a
synthetic recording (default 3000 frames, clips of 145 with overlap 2).

Device time: HIP events around `--inner` back-to-back passes, median over `--windows` windows after a warm-up of the same
shapes.  Host time: wall clock of one pass (it takes seconds; the body model runs batched over all frames there, which
flatters the host: the reference's loader calls it once per frame).  Recorded, not judged.

    python scripts/bench_clips.py [--out profiles/clips_timing.json] [--frames 3000]
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

import clips_ref as CR  # noqa: E402
import video_tree as VT  # noqa: E402
from oracle import frames as OF  # noqa: E402
from oracle import geometry as G  # noqa: E402
from rohm_amd.body_model import SMPLXLayer  # noqa: E402
from rohm_amd.data_loaders import clips, frames  # noqa: E402
from rohm_amd.utils import synth  # noqa: E402

DEV = 'cuda:0'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'clips_timing.json'))
    ap.add_argument('--frames', type=int, default=3000)
    ap.add_argument('--clip_len', type=int, default=145)
    ap.add_argument('--overlap', type=int, default=2)
    ap.add_argument('--inner', type=int, default=50)
    ap.add_argument('--windows', type=int, default=9)
    ap.add_argument('--skip_host', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_clips.py measures on the GPU; none found')
    N, L, ov = a.frames, a.clip_len, a.overlap
    g = np.random.Generator(np.random.PCG64(0))
    cam2world = VT._rigid(g, 0.3)
    p79 = VT._params(g, N, cam2world, 'z')
    params = {k: p79[:, lo:hi] for k, (lo, hi) in VT.PARAM_SLICES.items()}
    kp = np.concatenate([g.uniform(size=(N, 22, 2)) * np.array([1920., 1080.]), g.uniform(size=(N, 22, 1))], -1).astype(np.float32)
    mask = (g.uniform(size=(N, 25)) > 0.3).astype(np.float32)
    stats = synth.synthetic_stats(5)
    tensors = synth.synthetic_smplx_tensors(0)

    layer = SMPLXLayer.from_tensors(tensors).to(DEV)
    dparams = {k: torch.from_numpy(v).to(DEV) for k, v in params.items()}
    dkp, dmask = torch.from_numpy(kp).to(DEV), torch.from_numpy(mask).to(DEV)
    c2w = torch.from_numpy(cam2world.astype(np.float32)).to(DEV)

    def device_pass():
        jw, world = frames.frames_to_world(layer, dparams, c2w, DEV)
        built = clips.build_clips(jw, world, L, ov, 'z', stats=stats)
        jv, vv = clips.visibility_masks(dkp, dmask, L, ov)
        return built, jv, vv

    for _ in range(3):
        out = device_pass()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.inner):
            device_pass()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / a.inner)
    n_clips = int(out[0]['repr'].shape[0])
    res = {'frames': N, 'clip_len': L, 'overlap': ov, 'clips': n_clips, 'inner_passes': a.inner, 'windows': a.windows,
           'device_pass_ms_median': round(statistics.median(times), 4), 'device_pass_ms_min': round(min(times), 4),
           'device_pass_ms_max': round(max(times), 4),
           'device_clips_per_s': round(n_clips / (statistics.median(times) * 1e-3), 1)}

    if not a.skip_host:
        body = G.BodyModel(tensors)
        t = time.perf_counter()
        jw, world = OF.frames_to_world(body, params, cam2world.astype(np.float32))
        t_frames = time.perf_counter() - t
        ref = CR.build_clips(jw, world, L, ov, 'z', stats=stats)
        t_clips = time.perf_counter() - t - t_frames
        jv, vv = [], []
        for s in ref['starts']:
            m = CR.visibility_masks(kp[s:s + L], mask[s:s + L])
            jv.append(m[0]), vv.append(m[1])
        t_all = time.perf_counter() - t
        res.update({'host_pass_s': round(t_all, 3), 'host_frames_to_world_s': round(t_frames, 3),
                    'host_build_clips_s': round(t_clips, 3), 'host_masks_s': round(t_all - t_frames - t_clips, 3),
                    'host_threads': torch.get_num_threads(),
                    'max_abs_diff_repr': float(np.nanmax(np.abs(out[0]['repr'].cpu().numpy() - ref['repr']))),
                    'masks_equal': bool(np.array_equal(out[2].cpu().numpy(), np.stack(vv)))})
    print(json.dumps(res))
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
