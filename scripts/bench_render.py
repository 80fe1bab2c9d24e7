"""Timings of the colour renderer next to the depth renderer on the same bodies, and of one full AMASS evaluation frame
(three body scenes on the floor, two skeleton scenes, compositing), at 1920 x 1080.  Recorded, not judged: there is no
earlier colour path to compare with; the depth renderer on the same commit is the yardstick.

Each figure: warm-up calls of the same shape, then the median of `--runs` device-synchronised runs (HIP events).

    python scripts/bench_render.py [--out profiles/render_bench.json] [--runs 7]
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

import raster_ref as rr  # noqa: E402
import raster_scenes as rs  # noqa: E402
from rohm_amd import occlusion as occ  # noqa: E402
from rohm_amd import render as R  # noqa: E402
from rohm_amd.body_model import SMPLXLayer, lbs_forward, native_for  # noqa: E402

DEV = 'cuda:0'


def timed(fn, runs, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'render_bench.json'))
    ap.add_argument('--runs', type=int, default=7)
    args = ap.parse_args()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    n = rs.N_FRAMES
    res = {'image': list(rr.PROX_SIZE), 'frames': n, 'runs_per_figure': args.runs, 'statistic': 'median of runs, ms per frame'}

    tensors, faces = rs.sphere_body()
    body = SMPLXLayer.from_tensors(tensors).to(DEV)
    p = rs.walking_params(tensors, n)
    nat = native_for(body, torch.device(DEV))
    pose = torch.cat([dev(p['global_orient']).reshape(n, 1, 3), dev(p['body_pose']).reshape(n, 21, 3)], 1).contiguous()
    joints, verts = lbs_forward(nat, pose, 0, dev(p['betas']), dev(p['transl']))
    fd = dev(faces)
    adj = R.vertex_adjacency(faces, verts.shape[1])
    colors = dev(np.tile(np.uint8(R.MATERIALS['body_rec_vis']), (1, verts.shape[1], 1)))
    normals = R.vertex_normals(verts, fd, adj)
    res['body_faces'] = int(len(faces))

    def figure(key, fn, per=n):
        med, lo, hi = timed(fn, args.runs)
        res[key + '_ms_per_frame'] = round(med / per, 4)
        res[key + '_ms_per_frame_min_max'] = [round(lo / per, 4), round(hi / per, 4)]

    figure('depth_render', lambda: occ.depth_render(verts, fd, rr.PROX_CAM, rr.PROX_SIZE))
    figure('color_render_smooth_all_outputs', lambda: R.color_render(verts, fd, colors, rr.PROX_CAM, rr.PROX_SIZE, normals=normals,
                                                                     with_depth=True, with_face_id=True))
    figure('color_render_smooth_rgba_only', lambda: R.color_render(verts, fd, colors, rr.PROX_CAM, rr.PROX_SIZE, normals=normals))
    figure('vertex_normals', lambda: R.vertex_normals(verts, fd, adj))
    res['color_over_depth'] = round(res['color_render_smooth_all_outputs_ms_per_frame'] / res['depth_render_ms_per_frame'], 3)

    # one full AMASS frame: pred / input / gt bodies on the floor, pred / input skeletons, render_img, paste, flip.  The
    # walk is in camera coordinates; the floor is put under it (y down), which keeps what the tiles cost: all 5 000 are in view.
    floor_v, floor_f, floor_c = R.floor_mesh()
    floor_v = np.stack([floor_v[:, 0], np.full(len(floor_v), 1.2, np.float32), floor_v[:, 1] + 12.5], -1)
    scene = R._BodyScene(faces, verts.shape[1], torch.device(DEV), floor=(floor_v, floor_f[:, ::-1].copy(), floor_c))
    skel = R.SkeletonTemplate(torch.device(DEV))
    j22 = joints[:, :22].contiguous()
    contact = np.zeros((n, 4))
    c_rec, h_rec = R.skeleton_colors(n, 'lower', list(R.LOWER_MASK_JOINTS), True, add_contact=True, contact_lbl=contact)
    c_in, h_in = R.skeleton_colors(n, 'lower', list(R.LOWER_MASK_JOINTS), False)
    mat = lambda k: np.tile(np.uint8(R.MATERIALS[k]), (n, 1))

    def amass_frames():
        out = []
        for body_col, sk in (('body_rec_vis', (c_rec, h_rec)), ('body_noisy', (c_in, h_in)), ('body_gt', None)):
            img = R.requantize(scene.render(verts, mat(body_col), rr.PROX_CAM, rr.PROX_SIZE, None), 1.0)
            if sk is not None:
                img = R.paste(img, R.requantize(skel.render(j22, sk[0], sk[1], rr.PROX_CAM, rr.PROX_SIZE, None), 1.0))
            out.append(R.flip_lr(img))
        return out
    figure('amass_frame_5_scenes_and_compositing', amass_frames)
    res['skeleton_faces'] = int(len(skel.faces))
    res['floor_faces'] = int(len(floor_f))
    print(json.dumps(res))
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
