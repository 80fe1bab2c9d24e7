"""How long the export takes with and without the cross-fade: `export.export_params` with keep='first' (one launch of
`rohm_export_smplx`) and keep='blend' (one launch of `rohm_export_smplx_blend`), on the clips `DataloaderTrack` makes of the
synthetic ten-minute 60 fps track of scripts/bench_track.py (18 000 frames at 30 fps, clips of 145), once with the reference's
overlap of 2 frames and once with windows that share 32.  Both calls include the plan's upload, the kernel and the joints
recomputed from the exported parameters (`rohm_smplx_joints`).

A host clock around calls that end in a device synchronise, median over `--windows` windows of `--inner` calls after a
warm-up of the same shapes.  There is no target and no claimed speed-up: nobody runs this path in a loop, the file is the
record.

    python scripts/bench_export_blend.py [--out profiles/export_blend_bench.json] [--minutes 10] [--fps 60]
"""
import argparse
import json
import os
import pickle
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

import video_tree as VT  # noqa: E402
from bench_track import synthetic_track, timed  # noqa: E402
from rohm_amd.body_model import SMPLXLayer  # noqa: E402
from rohm_amd.data_loaders.track import DataloaderTrack, read_track  # noqa: E402
from rohm_amd.export import export_params, seam_summary  # noqa: E402
from rohm_amd.utils import synth  # noqa: E402

DEV = 'cuda:0'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'export_blend_bench.json'))
    ap.add_argument('--minutes', type=float, default=10.0)
    ap.add_argument('--fps', type=float, default=60.0)
    ap.add_argument('--clip_len', type=int, default=145)
    ap.add_argument('--overlaps', type=str, default='2,32')
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--windows', type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_export_blend.py measures on the GPU; none found')
    n = int(round(a.minutes * 60 * a.fps))
    rec = read_track(synthetic_track(n, a.fps))
    layer = SMPLXLayer.from_tensors(synth.synthetic_smplx_tensors(0)).to(DEV)
    res = {'source_frames': n, 'source_fps': a.fps, 'clip_len': a.clip_len, 'inner': a.inner, 'windows': a.windows, 'overlaps': {}}
    with tempfile.TemporaryDirectory() as logdir:
        mean, std = synth.synthetic_stats(5)
        for name, vec in (('AMASS_mean.pkl', mean), ('AMASS_std.pkl', std)):
            with open(os.path.join(logdir, name), 'wb') as f:
                pickle.dump(VT._stats_dict(vec), f)
        for overlap in [int(s) for s in a.overlaps.split(',') if s]:
            ds = DataloaderTrack(rec, body_model_path=layer, logdir=logdir, task='pose', clip_len=a.clip_len, overlap_len=overlap,
                                 use_scene_floor_height=False, device=DEV)
            x, tf = ds._device_data['motion_repr_noisy'], ds._device_data['transf_matrix']
            rows = int(x.shape[1])
            row = {'clips': len(ds), 'rows_per_clip': rows}
            for keep in ('first', 'blend'):
                plan = ds.export_plan(keep, rows=rows)
                plan, frames = plan[:-1], plan[-1]
                run = lambda: export_params(x, tf, layer, stats=ds, frame='scene', keep=keep, plan=plan)  # noqa: E731
                out = run()
                w = timed(run, a.inner, a.windows)
                row.update({f'{keep}_ms_median': round(statistics.median(w), 4), f'{keep}_ms_min': round(min(w), 4),
                            f'{keep}_ms_max': round(max(w), 4)})
                row['frames'] = frames
                if keep == 'blend':
                    seams, angle, dist = seam_summary(out)
                    row.update(seams=seams, blended_frames=int((out.frame_clip_b >= 0).sum()), largest_seam_angle_rad=angle,
                               largest_seam_dist_m=dist)
            res['overlaps'][str(overlap)] = row
    print(json.dumps(res))
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
