"""Timings of the depth renderer, the body probe and the whole joint-occlusion mask pass (rohm_amd.occlusion), one
device-synchronised run each after one warm-up of the same shape.  Recorded, not judged: there is no earlier
implementation to compare with, and the numpy restatement in tests/ is not a baseline.

    python scripts/bench_occlusion.py [--out profiles/occlusion_timing.json] [--frames 3000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import raster_ref as rr  # noqa: E402
import raster_scenes as rs  # noqa: E402
from rohm_amd import occlusion as occ  # noqa: E402
from rohm_amd.body_model import SMPLXLayer, lbs_forward, native_for  # noqa: E402

DEV = 'cuda:0'


def timed(fn):
    fn()                                   # warm-up of this shape: code objects, allocator
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'occlusion_timing.json'))
    ap.add_argument('--frames', type=int, default=3000)
    args = ap.parse_args()
    res = {'image': list(rr.PROX_SIZE), 'runs_per_figure': 1}
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)

    for n in (200, 708):                   # 79 202 and 999 698 triangles
        v, f = rr.height_field(n, 4.0)
        vd, fd = dev(v), dev(f)
        ms, img = timed(lambda: occ.depth_render(vd, fd, rr.PROX_CAM, rr.PROX_SIZE))
        res[f'scene_render_{len(f)}_tri_ms'] = round(ms, 3)
        res[f'scene_render_{len(f)}_tri_covered_px'] = int((img > 0).sum())

    # a body of SMPL-X's size (10 475 vertices, 20 908 faces there): 10 506 vertices, 20 808 faces
    tensors, faces = rs.sphere_body(0, 102, 102)
    body = SMPLXLayer.from_tensors(tensors).to(DEV)
    body.faces = faces
    p64 = rs.walking_params(tensors, rs.N_FRAMES)
    reps = -(-args.frames // rs.N_FRAMES)
    params = {k: dev(np.tile(v, (reps, 1))[:args.frames]) for k, v in p64.items()}
    sv, sf = rs.scene_mesh()
    scene = occ.depth_render(dev(sv), sf, rr.PROX_CAM, rr.PROX_SIZE)[0]

    n = min(1024, args.frames)
    nat = native_for(body, torch.device(DEV))
    pose = torch.cat([params['global_orient'][:n].reshape(n, 1, 3), params['body_pose'][:n].reshape(n, 21, 3)], 1).contiguous()
    joints, verts = lbs_forward(nat, pose, 0, params['betas'][:n].contiguous(), params['transl'][:n].contiguous())
    pix = occ.project_pixels(joints[:, :25].contiguous(), occ.camera_matrix(rr.PROX_CAM), None)
    fd = dev(faces)
    ms, _ = timed(lambda: occ.depth_probe(verts, fd, pix, rr.PROX_CAM, rr.PROX_SIZE))
    res['body_probe_frames'] = n
    res['body_probe_faces'] = int(len(faces))
    res['body_probe_ms'] = round(ms, 3)

    ms, mask = timed(lambda: occ.joint_occlusion_mask(body, params, scene, rr.PROX_CAM, [0.052, -0.044, 0.0009, 0.0016, 0.003]))
    res['mask_pass_frames'] = args.frames
    res['mask_pass_ms'] = round(ms, 3)
    res['mask_pass_frames_per_s'] = round(args.frames / (ms * 1e-3), 1)
    res['mask_pass_occluded_joints'] = int((mask == 0).sum())
    print(json.dumps(res))
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
