"""Depth rendering and PROX joint-occlusion masks on the device (csrc/raster.hip): what the reference's
`utils/get_occlusion_mask.py` does with pyrender, trimesh and OpenCV, without an OpenGL stack.

    python -m rohm_amd.occlusion --prox_root PROX --body_model_path data/body_models/smplx_model \\
        --init_body_path data/init_motions/init_prox_rgbd --save_mask_path mask_joint_prox \\
        --scene_name N0Sofa --seq_name N0Sofa_00034_01

writes `<save_mask_path>/<seq_name>/mask_joint.npy` ([n_frames, 25] float64, 1 = visible), the file the PROX driver and
PoseNet's training loop load.  The reference stops after the first 100 frames (`img_list[0:100]`); this tool takes all
frames unless `--max_frames 100` is given.

The coverage rule (pinhole camera in OpenCV axes, samples at pixel centres, nearest hit within [znear, zfar], two-sided
unless `cull_backfaces`) is stated in csrc/raster.hip and include/rohm_hip.h.  Parity with pyrender's rasteriser and
cv2.projectPoints themselves is not pinned by a fixture: neither is installed where this project is built.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import pickle
import sys

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr

ZNEAR, ZFAR = 0.05, 100.0                          # pyrender's DEFAULT_Z_NEAR / DEFAULT_Z_FAR
PROX_RENDER_CAM = (1060.53, 1060.38, 951.30, 536.77)      # get_occlusion_mask.py:64-69
PROX_SIZE = (1920, 1080)
N_MASK_JOINTS = 25                                 # "25 smplx main body joints", :137


# ---- PLY ------------------------------------------------------------------------------------------------------------
_PLY_TYPES = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'short': 'i2', 'int16': 'i2', 'ushort': 'u2',
              'uint16': 'u2', 'int': 'i4', 'int32': 'i4', 'uint': 'u4', 'uint32': 'u4', 'float': 'f4', 'float32': 'f4',
              'double': 'f8', 'float64': 'f8'}


def read_ply(path):
    """Minimal PLY reader: ascii or binary little-endian, `vertex` and `face` elements; vertex properties other than
    x, y, z are skipped, polygons are fanned into triangles.  -> (verts [V, 3] float32, faces [F, 3] int32)."""
    with open(path, 'rb') as f:
        data = f.read()
    end = data.find(b'end_header')
    if not data.startswith(b'ply') or end < 0:
        raise ValueError(f'{path}: not a PLY file')
    nl = data.index(b'\n', end) + 1
    fmt, elements = None, []
    for line in data[:end].decode('ascii', 'replace').splitlines():
        tok = line.split()
        if not tok:
            continue
        if tok[0] == 'format':
            fmt = tok[1]
        elif tok[0] == 'element':
            elements.append({'name': tok[1], 'count': int(tok[2]), 'props': []})
        elif tok[0] == 'property':
            if tok[1] == 'list':
                elements[-1]['props'].append((tok[4], 'list', _PLY_TYPES[tok[2]], _PLY_TYPES[tok[3]]))
            else:
                elements[-1]['props'].append((tok[2], _PLY_TYPES[tok[1]]))
    if fmt not in ('ascii', 'binary_little_endian'):
        raise ValueError(f'{path}: PLY format {fmt!r} is not supported (ascii and binary_little_endian are)')
    verts, faces = None, np.zeros((0, 3), np.int32)
    body = data[nl:]
    if fmt == 'ascii':
        rows = [ln.split() for ln in body.decode('ascii').splitlines() if ln.strip()]
        at = 0
        for el in elements:
            chunk = rows[at:at + el['count']]
            at += el['count']
            if el['name'] == 'vertex':
                names = [p[0] for p in el['props']]
                cols = [names.index(k) for k in ('x', 'y', 'z')]
                verts = np.array([[float(r[c]) for c in cols] for r in chunk], dtype=np.float32).reshape(-1, 3)
            elif el['name'] == 'face':
                polys = []
                for r in chunk:
                    k = int(r[0])
                    polys.append([int(v) for v in r[1:1 + k]])
                faces = _fan(polys)
        return verts, faces
    at = 0
    for el in elements:
        is_list = [len(p) == 4 for p in el['props']]
        if not any(is_list):
            dt = np.dtype([(p[0], '<' + p[1]) for p in el['props']])
            arr = np.frombuffer(body, dtype=dt, count=el['count'], offset=at)
            at += dt.itemsize * el['count']
            if el['name'] == 'vertex':
                verts = np.stack([arr['x'], arr['y'], arr['z']], axis=1).astype(np.float32)
            continue
        if el['name'] != 'face' or len(el['props']) != 1:
            raise ValueError(f'{path}: element {el["name"]!r} mixes list and scalar properties, which is not supported')
        _, _, ct, it = el['props'][0]
        ct, it = np.dtype('<' + ct), np.dtype('<' + it)
        if el['count'] == 0:
            continue
        # the common case, all triangles, in one view; anything else polygon by polygon
        rec = np.dtype([('n', ct), ('v', it, (3,))])
        whole = el['count'] * rec.itemsize
        tri = np.frombuffer(body, dtype=rec, count=el['count'], offset=at) if at + whole <= len(body) else None
        if tri is not None and bool((tri['n'] == 3).all()):
            faces = tri['v'].astype(np.int32)
            at += whole
        else:
            polys = []
            for _ in range(el['count']):
                k = int(np.frombuffer(body, dtype=ct, count=1, offset=at)[0])
                at += ct.itemsize
                polys.append(np.frombuffer(body, dtype=it, count=k, offset=at).tolist())
                at += it.itemsize * k
            faces = _fan(polys)
    if verts is None:
        raise ValueError(f'{path}: no vertex element')
    return verts, faces


def _fan(polys):
    tris = [[p[0], p[i], p[i + 1]] for p in polys for i in range(1, len(p) - 1)]
    return np.asarray(tris, dtype=np.int32).reshape(-1, 3)


# ---- device calls ---------------------------------------------------------------------------------------------------
def _cam4(cam):
    fx, fy, cx, cy = (float(v) for v in cam)
    return fx, fy, cx, cy


def _transform_arg(transform):
    if transform is None:
        return None
    m = np.ascontiguousarray(np.asarray(transform.detach().cpu() if torch.is_tensor(transform) else transform,
                                        dtype=np.float32).reshape(4, 4))
    return (C.c_float * 16)(*m.ravel().tolist())


def _lens_args(camera_mtx, dist_coeffs):
    k = np.asarray(camera_mtx, dtype=np.float64).reshape(3, 3)
    d = np.zeros(5, np.float64) if dist_coeffs is None else np.asarray(dist_coeffs, dtype=np.float64).ravel()
    if d.size != 5:
        raise ValueError(f'five distortion coefficients (k1, k2, p1, p2, k3) expected, got {d.size}')
    return (C.c_double * 9)(*k.ravel().tolist()), (C.c_double * 5)(*d.tolist())


def camera_matrix(cam):
    """(fx, fy, cx, cy) -> 3 x 3 matrix; a 3 x 3 matrix passes through."""
    a = np.asarray(cam, dtype=np.float64)
    if a.size == 9:
        return a.reshape(3, 3)
    fx, fy, cx, cy = a.ravel()
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dtype=np.float64)


def _mesh_args(verts, faces):
    _lib.require_hip(verts)
    if verts.dim() == 2:
        verts = verts.unsqueeze(0)
    verts = verts.float().contiguous()
    if not torch.is_tensor(faces):
        faces = torch.from_numpy(np.ascontiguousarray(np.asarray(faces).astype(np.int32)))
    faces = faces.to(device=verts.device, dtype=torch.int32).reshape(-1, 3).contiguous()
    return verts, faces


def depth_render(verts, faces, cam, size, transform=None, cull_backfaces=False, znear=ZNEAR, zfar=ZFAR):
    """Depth images [n_mesh, H, W] float32 (0 = nothing hit) of meshes `verts` [n_mesh, V, 3] (or [V, 3]) sharing the
    face list `faces` [F, 3].  cam = (fx, fy, cx, cy), size = (W, H); `transform`: optional 4 x 4 rigid transform into
    camera space, applied on the device.  Two-sided unless `cull_backfaces` (pyrender culls by default; scene scans are
    open surfaces, so the two differ where a surface is seen from behind)."""
    verts, faces = _mesh_args(verts, faces)
    fx, fy, cx, cy = _cam4(cam)
    W, H = int(size[0]), int(size[1])
    n_mesh, V, F = verts.shape[0], verts.shape[1], faces.shape[0]
    dev = verts.device
    out = torch.empty(n_mesh, H, W, dtype=torch.float32, device=dev)
    n = lib().rohm_depth_workspace_bytes(n_mesh, F, W, H)
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    check(lib().rohm_depth_render(ptr(verts), ptr(faces), n_mesh, V, F, _transform_arg(transform), fx, fy, cx, cy, W, H,
                                  znear, zfar, int(bool(cull_backfaces)), ptr(out), ptr(ws), ws.numel(), stream_ptr(dev)),
          'rohm_depth_render')
    return out


def depth_probe(verts, faces, pixels, cam, size, transform=None, cull_backfaces=False, znear=ZNEAR, zfar=ZFAR):
    """The renderer's depth at `pixels` [n_mesh, P, 2] int32 (x, y) only -> [n_mesh, P] float32, bit for bit what
    `depth_render` holds there; 0 for a pixel outside the image."""
    verts, faces = _mesh_args(verts, faces)
    _lib.require_hip(pixels)
    fx, fy, cx, cy = _cam4(cam)
    W, H = int(size[0]), int(size[1])
    n_mesh, V, F = verts.shape[0], verts.shape[1], faces.shape[0]
    pixels = pixels.to(torch.int32).reshape(n_mesh, -1, 2).contiguous()
    P = pixels.shape[1]
    out = torch.empty(n_mesh, P, dtype=torch.float32, device=verts.device)
    check(lib().rohm_depth_probe(ptr(verts), ptr(faces), n_mesh, V, F, _transform_arg(transform), fx, fy, cx, cy, W, H,
                                 znear, zfar, int(bool(cull_backfaces)), ptr(pixels), P, ptr(out), stream_ptr(verts.device)),
          'rohm_depth_probe')
    return out


def project_pixels(joints, camera_mtx, dist_coeffs=None):
    """cv2.projectPoints (zero rvec / tvec) followed by astype(int): joints [N, J, 3] -> pixels [N, J, 2] int32."""
    _lib.require_hip(joints)
    joints = joints.float().contiguous()
    N, J = joints.shape[0], joints.shape[1]
    k, d = _lens_args(camera_matrix(camera_mtx), dist_coeffs)
    pix = torch.empty(N, J, 2, dtype=torch.int32, device=joints.device)
    check(lib().rohm_project_pixels(ptr(joints), k, d, N, J, ptr(pix), stream_ptr(joints.device)), 'rohm_project_pixels')
    return pix


def mask_from_depths(joints, scene_depth, body_depth, camera_mtx, dist_coeffs=None, thr=0.1):
    """The decision of get_occlusion_mask.py:138-143 -> [N, J] float32, 1 = visible."""
    _lib.require_hip(joints, scene_depth, body_depth)
    joints, scene_depth, body_depth = joints.float().contiguous(), scene_depth.float().contiguous(), body_depth.float().contiguous()
    N, J = joints.shape[0], joints.shape[1]
    H, W = scene_depth.shape[-2], scene_depth.shape[-1]
    k, d = _lens_args(camera_matrix(camera_mtx), dist_coeffs)
    mask = torch.empty(N, J, dtype=torch.float32, device=joints.device)
    check(lib().rohm_joint_occlusion_mask(ptr(joints), k, d, ptr(scene_depth), W, H, ptr(body_depth), float(thr), N, J,
                                          ptr(mask), stream_ptr(joints.device)), 'rohm_joint_occlusion_mask')
    return mask


def joint_occlusion_mask(body_model, smplx_params, scene_depth, cam, dist_coeffs, thr=0.1, proj_camera_mtx=None,
                         n_joints=N_MASK_JOINTS, chunk=1024, cull_backfaces=False):
    """Visibility of the first 25 SMPL-X joints of every frame -> [N, 25] float32 (1 = visible).

    `smplx_params`: transl [N, 3], global_orient [N, 3], body_pose [N, 63], betas [N, 10] (camera space, as PROX's
    fits are); hands, jaw and eyes stay at rest, as in the script.  `scene_depth` [H, W]: the static scene rendered with
    `depth_render` and the same `cam` = (fx, fy, cx, cy), which also probes the body.  The joints are projected with
    `proj_camera_mtx` (3 x 3, default: `cam`) and `dist_coeffs` (k1, k2, p1, p2, k3) -- the script renders with fixed
    intrinsics and projects with calibration/Color.json's.  Needs `faces` on the body-model layer."""
    from .body_model import lbs_forward, native_for
    faces = getattr(body_model, 'faces', None)
    if faces is None:
        raise _lib.RohmHipError('joint_occlusion_mask needs the body model\'s faces (SMPLXLayer.from_npz keeps them)')
    _lib.require_hip(scene_depth)
    dev = scene_depth.device
    nat = native_for(body_model, dev)
    f32 = lambda k: torch.as_tensor(smplx_params[k]).to(device=dev, dtype=torch.float32)
    transl, betas = f32('transl').reshape(-1, 3), f32('betas')
    N = transl.shape[0]
    betas = betas.reshape(N, -1).contiguous()
    pose = torch.cat([f32('global_orient').reshape(N, 1, 3), f32('body_pose').reshape(N, -1, 3)], dim=1).contiguous()
    faces_d = torch.as_tensor(np.asarray(faces).astype(np.int32)).to(dev).reshape(-1, 3).contiguous()
    H, W = scene_depth.shape[-2], scene_depth.shape[-1]
    scene_depth = scene_depth.reshape(H, W)
    kmat = camera_matrix(cam if proj_camera_mtx is None else proj_camera_mtx)
    out = torch.empty(N, n_joints, dtype=torch.float32, device=dev)
    for s0 in range(0, N, chunk):
        s1 = min(N, s0 + chunk)
        joints, verts = lbs_forward(nat, pose[s0:s1], 0, betas[s0:s1], transl[s0:s1].contiguous())
        j = joints[:, :n_joints].contiguous()
        pix = project_pixels(j, kmat, dist_coeffs)
        body = depth_probe(verts, faces_d, pix, cam, (W, H), cull_backfaces=cull_backfaces)
        out[s0:s1] = mask_from_depths(j, scene_depth, body, kmat, dist_coeffs, thr)
    return out


# ---- the tool -------------------------------------------------------------------------------------------------------
def _frame_names(prox_root, init_body_path, seq_name):
    """The script walks recordings/<seq>/Color (:93-99); without the images, the fitted frames themselves."""
    img_folder = os.path.join(prox_root, 'recordings', seq_name, 'Color')
    if os.path.isdir(img_folder):
        names = sorted(os.listdir(img_folder))
        return [n[0:-4] for n in names if n.endswith('.png') or n.endswith('.jpg') and not n.startswith('.')]
    results = os.path.join(init_body_path, seq_name, 'results')
    return sorted(n for n in os.listdir(results) if os.path.isfile(os.path.join(results, n, '000.pkl')))


def _body_model_file(body_model_path):
    for cand in (body_model_path, os.path.join(body_model_path, 'SMPLX_NEUTRAL.npz'),
                 os.path.join(body_model_path, 'smplx', 'SMPLX_NEUTRAL.npz')):
        if os.path.isfile(cand):
            return cand
    raise FileNotFoundError(f'no SMPLX_NEUTRAL.npz under {body_model_path}')


def main(argv=None):
    from .body_model import SMPLXLayer
    ap = argparse.ArgumentParser(description='PROX joint-occlusion masks (utils/get_occlusion_mask.py) on the device')
    ap.add_argument('--prox_root', type=str, default='/mnt/hdd/PROX')
    ap.add_argument('--body_model_path', type=str, default='../data/body_models/smplx_model')
    ap.add_argument('--init_body_path', type=str, default='../data/init_motions/init_prox_rgbd')
    ap.add_argument('--save_mask_path', type=str, default='../mask_joint_prox')
    ap.add_argument('--scene_name', type=str, default='N0Sofa')
    ap.add_argument('--seq_name', type=str, default='N0Sofa_00034_01')
    ap.add_argument('--max_frames', type=int, default=0, help='0 = all frames; 100 reproduces the reference script')
    ap.add_argument('--cull_backfaces', action='store_true', help='drop back faces as pyrender does')
    ap.add_argument('--device', type=str, default='cuda:0')
    args = ap.parse_args(argv)
    dev = torch.device(args.device)

    with open(os.path.join(args.prox_root, 'cam2world', args.scene_name + '.json')) as f:
        cam2world = np.array(json.load(f), dtype=np.float64)
    with open(os.path.join(args.prox_root, 'calibration', 'Color.json')) as f:
        color_cam = json.load(f)
    sv, sf = read_ply(os.path.join(args.prox_root, 'scenes', args.scene_name + '.ply'))
    scene_depth = depth_render(torch.from_numpy(sv).to(dev), sf, PROX_RENDER_CAM, PROX_SIZE,
                               transform=np.linalg.inv(cam2world), cull_backfaces=args.cull_backfaces)[0]

    names = _frame_names(args.prox_root, args.init_body_path, args.seq_name)
    if args.max_frames > 0:
        names = names[:args.max_frames]
    if not names:
        raise SystemExit('no frames found')
    keys = ('transl', 'global_orient', 'body_pose', 'betas')
    rows = {k: [] for k in keys}
    for n in names:
        with open(os.path.join(args.init_body_path, args.seq_name, 'results', n, '000.pkl'), 'rb') as f:
            d = pickle.load(f, encoding='latin1')
        for k in keys:
            rows[k].append(np.asarray(d[k], dtype=np.float32).reshape(-1))
    params = {k: torch.from_numpy(np.stack(v)) for k, v in rows.items()}
    params['betas'] = params['betas'][:, :10]

    body = SMPLXLayer.from_npz(_body_model_file(args.body_model_path)).to(dev)
    mask = joint_occlusion_mask(body, params, scene_depth, PROX_RENDER_CAM, color_cam['k'],
                                proj_camera_mtx=color_cam['camera_mtx'], cull_backfaces=args.cull_backfaces)
    out_dir = os.path.join(args.save_mask_path, args.seq_name)
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, 'mask_joint.npy')
    np.save(out, mask.cpu().numpy().astype(np.float64))      # the script stacks np.ones([25]) rows: float64
    print(f'[rohm_amd.occlusion] {len(names)} frames, {int((mask == 0).sum())} occluded joints -> {out}')
    return 0


if __name__ == '__main__':
    sys.exit(main())
