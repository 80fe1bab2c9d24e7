"""Evaluation pictures on the device (csrc/shade.hip): the `--render` path of the reference's eval_amass_full.py:277-395 and
eval_prox_egobody.py:373-451 (utils/render_util.py) without pyrender, trimesh, an OpenGL context, cv2 or PIL.

Shaded SMPL-X bodies, the 22-joint skeleton with occluded joints and foot contacts coloured, the checkerboard floor, the
scripts' compositing (render_img, Image.paste, render_img_overlay, the left-right flip) and a PNG writer from the standard
library.  The shading rule -- the depth renderer's coverage, nearest surface with the lowest face index on ties,
perspective-correct interpolation, ambient + Lambert under one directional light along the viewing axis -- is stated in
include/rohm_hip.h.  Stated differences from pyrender: no specular term, no sRGB curve, nothing blended behind a
translucent surface.  Nothing is pinned to pyrender, which is not installed where this project is built.

Torch only holds buffers and indexes them; the host builders (templates, floor, adjacency, colour tables) are numpy and
run once.
"""
from __future__ import annotations

import math
import os
import struct
import zlib

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr
from .occlusion import ZFAR, ZNEAR, _cam4, _mesh_args, _transform_arg

AMBIENT = 0.3                       # create_pyrender_scene: ambient_light=(0.3, 0.3, 0.3)
DIFFUSE = 3.0 / math.pi             # DirectionalLight(intensity=3.0) on a non-metallic material: Lambert's albedo / pi
JOINT_RADIUS, LIMB_RADIUS = 0.025, 0.01
AMASS_CAM = (1060.53, 1060.38, 960.0, 540.0)                 # eval_amass_full.py:288
AMASS_CAM_TRANS = ((0, 0, -1, 5), (-1, 0, 0, 1), (0, -1, 0, 1), (0, 0, 0, 1))      # :289-292
AMASS_SIZE = (1920, 1080)
FULL_MASK_START, CLIP_LEN_AMASS = 65, 145                    # :83-85

# utils/render_util.py:7-56, baseColorFactor x 255
MATERIALS = {
    'body_rec_vis': (66, 149, 245, 255), 'body_rec_occ': (212, 189, 102, 255), 'body_noisy': (198, 226, 255, 255),
    'body_gt': (255, 102, 102, 255), 'joint_vis': (6, 75, 255, 255), 'joint_occ': (222, 177, 4, 255),
    'skel_vis': (90, 135, 247, 255), 'skel_occ': (219, 199, 123, 255), 'contact_1': (0, 139, 0, 255),
    'contact_0': (205, 0, 0, 255),
}
FLOOR_COLORS = ((0.8, 0.9, 0.9), (0.6, 0.7, 0.7))            # create_floor
# utils/other_utils.py:62-89: the 21 child-parent edges of the 22-joint body
LIMBS_BODY_SMPL = ((15, 12), (12, 13), (13, 16), (16, 18), (18, 20), (12, 14), (14, 17), (17, 19), (19, 21), (12, 9), (9, 6),
                   (6, 3), (3, 0), (0, 1), (1, 4), (4, 7), (7, 10), (0, 2), (2, 5), (5, 8), (8, 11))
CONTACT_IDX = {7: 0, 10: 1, 8: 2, 11: 3}
N_JOINTS, N_LIMBS = 22, 21
LOWER_BODY_PARTS = ('leftLeg', 'rightLeg', 'leftToeBase', 'rightToeBase', 'leftFoot', 'rightFoot', 'leftUpLeg', 'rightUpLeg')
LOWER_MASK_JOINTS = (1, 2, 4, 5, 7, 8, 10, 11)


# ---- host builders --------------------------------------------------------------------------------------------------
def icosphere(subdivisions=3):
    """Unit icosphere -> (verts [V, 3] float32, faces [F, 3] int32), V = 10 * 4^s + 2, F = 20 * 4^s, wound outward."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(int(subdivisions)):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.asarray(v, dtype=np.float32), np.asarray(f, dtype=np.int32)


def cylinder(sections=32):
    """Unit cylinder, axis z from 0 to 1, radius 1, capped -> (verts [2 + 2 s, 3] float32, faces [4 s, 3] int32), wound outward."""
    s = int(sections)
    ang = np.arange(s) * (2.0 * np.pi / s)
    ring = np.stack([np.cos(ang), np.sin(ang)], -1)
    v = np.concatenate([[[0, 0, 0], [0, 0, 1]], np.concatenate([ring, np.zeros((s, 1))], 1), np.concatenate([ring, np.ones((s, 1))], 1)])
    i = np.arange(s)
    j = (i + 1) % s
    b, t = 2 + i, 2 + s + i
    bj, tj = 2 + j, 2 + s + j
    f = np.concatenate([np.stack([np.zeros(s, int), bj, b], -1), np.stack([np.ones(s, int), t, tj], -1),
                        np.stack([b, bj, tj], -1), np.stack([b, tj, t], -1)])
    return v.astype(np.float32), f.astype(np.int32)


def floor_mesh(trans=None):
    """create_floor: a 25 m checkerboard of 0.5 m tiles at z = 0, every tile with its own four vertices -> (verts [10000, 3]
    float32, faces [5000, 3] int32, colors [10000, 4] uint8).  `trans`: the mesh is moved by inv(trans), as the script does;
    None leaves it in world coordinates (the renderer's `transform` then moves it with everything else)."""
    tile, length = 0.5, 25.0
    radius, n = length / 2.0, int(length / 0.5)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
    x0, y0 = -radius + j * tile, radius - i * tile
    corners = np.stack([np.stack([x0, y0], -1), np.stack([x0, y0 - tile], -1), np.stack([x0 + tile, y0 - tile], -1),
                        np.stack([x0 + tile, y0], -1)], 2)                                  # [n, n, 4, 2]
    v = np.concatenate([corners, np.zeros(corners.shape[:-1] + (1,))], -1).reshape(-1, 3)
    base = 4 * (i * n + j).reshape(-1, 1, 1)
    f = (base + np.array([[0, 1, 3], [1, 2, 3]])[None]).reshape(-1, 3)
    c0, c1 = (np.round(np.array(c + (1.0,)) * 255).astype(np.uint8) for c in FLOOR_COLORS)
    even = ((i % 2) == (j % 2)).reshape(-1)
    colors = np.repeat(np.where(even[:, None], c0[None], c1[None]), 4, axis=0)
    if trans is not None:
        m = np.linalg.inv(np.asarray(trans, dtype=np.float64))
        v = v @ m[:3, :3].T + m[:3, 3]
    return v.astype(np.float32), f.astype(np.int32), np.ascontiguousarray(colors, dtype=np.uint8)


def merge(*meshes):
    """Meshes (verts [V, 3], faces [F, 3], colors [V, 4] uint8) -> one mesh with the face indices shifted."""
    vs, fs, cs, off = [], [], [], 0
    for v, f, c in meshes:
        vs.append(np.asarray(v, dtype=np.float32))
        fs.append(np.asarray(f, dtype=np.int32) + off)
        cs.append(np.asarray(c, dtype=np.uint8).reshape(len(v), 4))
        off += len(v)
    return np.concatenate(vs), np.concatenate(fs).astype(np.int32), np.concatenate(cs)


def vertex_adjacency(faces, V):
    """Vertex -> face adjacency in CSR form: (offsets [V + 1], face_ids [3 F]) int32, each vertex's faces in list order."""
    flat = np.asarray(faces, dtype=np.int64).reshape(-1)
    if flat.size and (flat.min() < 0 or flat.max() >= V):
        raise ValueError('face index outside [0, V)')
    order = np.argsort(flat, kind='stable')
    offsets = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=V))])
    return offsets.astype(np.int32), (order // 3).astype(np.int32)


def skeleton_colors(n_frames, mask_scheme, mask_joint_id=None, add_occ_joints=True, start=0, end=0, add_contact=False,
                    contact_lbl=None):
    """create_pyrender_skel's materials and omissions for `n_frames` frames -> (colors [T, 43, 4] uint8, hide [T, 43] uint8):
    22 joints, then the 21 limbs.  mask_scheme 'lower' | 'video' take `mask_joint_id` (joint ids, or a [T, 22] boolean array
    of occluded joints per frame); 'full' takes the [start, end) frame window.  `contact_lbl` [T, 4]: labels of joints
    7, 10, 8, 11 (with `add_contact`)."""
    if mask_scheme not in ('lower', 'video', 'full'):
        raise ValueError(f'unknown mask_scheme {mask_scheme!r}')
    T = int(n_frames)
    M = {k: np.asarray(v, dtype=np.uint8) for k, v in MATERIALS.items()}
    occ = np.zeros((T, N_JOINTS), bool)
    if mask_scheme != 'full' and mask_joint_id is not None:
        m = np.asarray(mask_joint_id)
        if m.dtype == bool:
            occ[:] = m.reshape(-1, N_JOINTS)
        elif m.size:
            occ[:, m.astype(np.int64).reshape(-1)] = True
    t = np.arange(T)
    in_window = (t >= start) & (t < end)
    joint_occ = np.broadcast_to(in_window[:, None], (T, N_JOINTS)) if mask_scheme == 'full' else occ
    colors = np.empty((T, N_JOINTS + N_LIMBS, 4), np.uint8)
    hide = np.zeros((T, N_JOINTS + N_LIMBS), np.uint8)
    colors[:, :N_JOINTS] = np.where(joint_occ[..., None], M['joint_occ'], M['joint_vis'])
    if add_contact:
        lbl = np.asarray(contact_lbl).reshape(T, 4)
        for j, k in CONTACT_IDX.items():
            colors[:, j] = np.where((lbl[:, k] == 1)[:, None], M['contact_1'], M['contact_0'])
    a, b = np.asarray(LIMBS_BODY_SMPL).T
    limb_occ = np.broadcast_to(in_window[:, None], (T, N_LIMBS)) if mask_scheme == 'full' else (occ[:, a] | occ[:, b])
    colors[:, N_JOINTS:] = np.where(limb_occ[..., None], M['joint_occ'], M['skel_vis'])      # joint_occ, as the script has it
    if mask_scheme != 'full' and not add_occ_joints:
        hide[:, :N_JOINTS] = occ
        hide[:, N_JOINTS:] = limb_occ
    return colors, hide


def write_png(path, image):
    """uint8 [H, W, 3] or [H, W, 4] -> an 8-bit RGB / RGBA PNG, with the standard library only."""
    a = np.ascontiguousarray(image.detach().cpu().numpy() if torch.is_tensor(image) else image)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (3, 4):
        raise ValueError(f'write_png takes uint8 [H, W, 3 | 4], got {a.dtype} {a.shape}')
    H, W, C = a.shape
    raw = np.concatenate([np.zeros((H, 1), np.uint8), a.reshape(H, W * C)], axis=1).tobytes()      # filter 0 on every row

    def chunk(tag, data):
        return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xffffffff)
    blob = b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, 8, 6 if C == 4 else 2, 0, 0, 0)) + \
        chunk(b'IDAT', zlib.compress(raw, 3)) + chunk(b'IEND', b'')
    with open(path, 'wb') as f:
        f.write(blob)


# ---- device calls ---------------------------------------------------------------------------------------------------
def _u8(t, channels=None):
    _lib.require_hip(t)
    if t.dtype != torch.uint8:
        raise TypeError(f'uint8 image expected, got {t.dtype}')
    if channels is not None and t.shape[-1] not in channels:
        raise ValueError(f'{" or ".join(map(str, channels))} channels expected, got shape {tuple(t.shape)}')
    return t.contiguous()


def vertex_normals(verts, faces, adjacency=None):
    """Smooth, area-weighted vertex normals [n_mesh, V, 3] of `verts` [n_mesh, V, 3] (or [V, 3]); `adjacency`: what
    `vertex_adjacency(faces, V)` returns (built here when None).  A vertex without a face gets (0, 0, 0)."""
    verts, faces_d = _mesh_args(verts, faces)
    n_mesh, V, F = verts.shape[0], verts.shape[1], faces_d.shape[0]
    if adjacency is None:
        adjacency = vertex_adjacency(faces_d.cpu().numpy(), V)
    off, ids = (torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).to(device=verts.device, dtype=torch.int32).contiguous()
                for a in adjacency)
    if off.numel() != V + 1 or ids.numel() != 3 * F:
        raise ValueError('adjacency does not belong to this face list')
    out = torch.empty_like(verts)
    check(lib().rohm_vertex_normals(ptr(verts), ptr(faces_d), ptr(off), ptr(ids), n_mesh, V, F, ptr(out), stream_ptr(verts.device)),
          'rohm_vertex_normals')
    return out


def color_render(verts, faces, colors, cam, size, normals=None, transform=None, cull_backfaces=False, ambient=AMBIENT,
                 diffuse=DIFFUSE, znear=ZNEAR, zfar=ZFAR, with_depth=False, with_face_id=False):
    """Shaded images uint8 [n_mesh, H, W, 4] of meshes `verts` [n_mesh, V, 3] sharing `faces` [F, 3].  `colors`: uint8 RGBA
    per vertex, [V, 4] / [1, V, 4] for all meshes or [n_mesh, V, 4]; `normals` [n_mesh, V, 3] (smooth) or None (flat).
    cam, size, transform, cull_backfaces as in `occlusion.depth_render`.  With `with_depth` / `with_face_id` the result is
    (rgba, depth [n_mesh, H, W] float32 or None, face_id [n_mesh, H, W] int32 or None); the depth equals
    `depth_render`'s bit for bit, face_id is -1 where nothing is hit."""
    verts, faces_d = _mesh_args(verts, faces)
    fx, fy, cx, cy = _cam4(cam)
    W, H = int(size[0]), int(size[1])
    n_mesh, V, F = verts.shape[0], verts.shape[1], faces_d.shape[0]
    dev = verts.device
    colors = _u8(colors, (4,))
    if colors.dim() == 2:
        colors = colors.unsqueeze(0)
    if colors.shape[1:] != (V, 4) or colors.shape[0] not in (1, n_mesh):
        raise ValueError(f'colors must be [{n_mesh} or 1, {V}, 4], got {tuple(colors.shape)}')
    per_mesh = int(colors.shape[0] == n_mesh and n_mesh > 1)
    if normals is not None:
        _lib.require_hip(normals)
        normals = normals.float().reshape(n_mesh, V, 3).contiguous()
    rgba = torch.empty(n_mesh, H, W, 4, dtype=torch.uint8, device=dev)
    depth = torch.empty(n_mesh, H, W, dtype=torch.float32, device=dev) if with_depth else None
    face_id = torch.empty(n_mesh, H, W, dtype=torch.int32, device=dev) if with_face_id else None
    ws = torch.empty(lib().rohm_color_workspace_bytes(n_mesh, F, W, H), dtype=torch.uint8, device=dev)
    check(lib().rohm_color_render(ptr(verts), ptr(faces_d), n_mesh, V, F, _transform_arg(transform), fx, fy, cx, cy, W, H, znear,
                                  zfar, int(bool(cull_backfaces)), ptr(normals), ptr(colors), per_mesh, float(ambient),
                                  float(diffuse), ptr(rgba), ptr(depth), ptr(face_id), ptr(ws), ws.numel(), stream_ptr(dev)),
          'rohm_color_render')
    return (rgba, depth, face_id) if (with_depth or with_face_id) else rgba


def skeleton_mesh(joints, sphere, cyl, limbs=LIMBS_BODY_SMPL, hide=None, r_joint=JOINT_RADIUS, r_limb=LIMB_RADIUS):
    """Spheres at the joints and cylinders along the limbs -> verts [N, J Vs + L Vc, 3].  joints [N, J, 3]; `sphere` [Vs, 3]
    and `cyl` [Vc, 3] unit templates; `hide` [N, J + L] bytes: hidden primitives collapse onto their first joint."""
    _lib.require_hip(joints)
    joints = joints.float().contiguous()
    dev = joints.device
    N, J = joints.shape[0], joints.shape[1]
    f32 = lambda a: torch.as_tensor(a).to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
    sphere, cyl = f32(sphere), f32(cyl)
    limbs_d = torch.as_tensor(np.asarray(limbs, dtype=np.int32) if not torch.is_tensor(limbs) else limbs).to(device=dev, dtype=torch.int32)
    limbs_d = limbs_d.reshape(-1, 2).contiguous()
    L, Vs, Vc = limbs_d.shape[0], sphere.shape[0], cyl.shape[0]
    if hide is not None:
        hide = torch.as_tensor(hide).to(device=dev, dtype=torch.uint8).contiguous()
        if hide.shape != (N, J + L):
            raise ValueError(f'hide must be [{N}, {J + L}], got {tuple(hide.shape)}')
    out = torch.empty(N, J * Vs + L * Vc, 3, dtype=torch.float32, device=dev)
    check(lib().rohm_skeleton_mesh(ptr(joints), N, J, ptr(sphere), Vs, ptr(cyl), Vc, ptr(limbs_d), L, float(r_joint), float(r_limb),
                                   ptr(hide), ptr(out), stream_ptr(dev)), 'rohm_skeleton_mesh')
    return out


def requantize(rgba, alpha=1.0):
    """render_img's round trip on uint8 RGBA images [..., 4]: / 255 in float32, alpha channel x `alpha`, x 255, truncate."""
    rgba = _u8(rgba, (4,))
    out = torch.empty_like(rgba)
    check(lib().rohm_image_requantize(ptr(rgba), float(alpha), rgba.numel() // 4, ptr(out), stream_ptr(rgba.device)),
          'rohm_image_requantize')
    return out


def paste(dst, src_rgba):
    """Image.paste(src, (0, 0), src) onto RGB or RGBA images `dst` [..., 3 | 4] -> a new tensor."""
    dst, src = _u8(dst, (3, 4)).clone(), _u8(src_rgba, (4,))
    if dst.shape[:-1] != src.shape[:-1]:
        raise ValueError(f'paste: {tuple(dst.shape)} and {tuple(src.shape)} differ in size')
    check(lib().rohm_image_paste(ptr(dst), dst.shape[-1], ptr(src), src.numel() // 4, stream_ptr(dst.device)), 'rohm_image_paste')
    return dst


def overlay(dst_rgb, src_rgba):
    """render_img_overlay: `src`'s rgb where its alpha > 0, `dst_rgb` elsewhere -> [..., 3]."""
    dst, src = _u8(dst_rgb, (3,)), _u8(src_rgba, (4,))
    if dst.shape[:-1] != src.shape[:-1]:
        raise ValueError(f'overlay: {tuple(dst.shape)} and {tuple(src.shape)} differ in size')
    out = torch.empty_like(dst)
    check(lib().rohm_image_overlay(ptr(dst), ptr(src), src.numel() // 4, ptr(out), stream_ptr(dst.device)), 'rohm_image_overlay')
    return out


def flip_lr(img):
    """Image.FLIP_LEFT_RIGHT on images [..., H, W, C]."""
    img = _u8(img, (1, 2, 3, 4))
    Wd, Ch = img.shape[-2], img.shape[-1]
    out = torch.empty_like(img)
    check(lib().rohm_image_flip_lr(ptr(img), img.numel() // (Wd * Ch), Wd, Ch, ptr(out), stream_ptr(img.device)), 'rohm_image_flip_lr')
    return out


# ---- scenes ---------------------------------------------------------------------------------------------------------
class SkeletonTemplate:
    """The fixed part of the skeleton's mesh: templates, face list, adjacency and the primitive every vertex belongs to."""

    def __init__(self, device, subdivisions=3, sections=32):
        sv, sf = icosphere(subdivisions)
        cv, cf = cylinder(sections)
        Vs, Vc = len(sv), len(cv)
        self.sphere, self.cyl = sv, cv
        faces = [sf + j * Vs for j in range(N_JOINTS)] + [cf + N_JOINTS * Vs + l * Vc for l in range(N_LIMBS)]
        self.faces = np.concatenate(faces).astype(np.int32)
        self.n_verts = N_JOINTS * Vs + N_LIMBS * Vc
        self.adjacency = vertex_adjacency(self.faces, self.n_verts)
        prim = np.concatenate([np.repeat(np.arange(N_JOINTS), Vs), N_JOINTS + np.repeat(np.arange(N_LIMBS), Vc)])
        self.prim = torch.from_numpy(prim).to(device)
        self.faces_d = torch.from_numpy(self.faces).to(device)

    def render(self, joints, colors, hide, cam, size, transform):
        """joints [T, 22, 3] device, colors [T, 43, 4] / hide [T, 43] from `skeleton_colors` -> rgba [T, H, W, 4]."""
        verts = skeleton_mesh(joints, self.sphere, self.cyl, hide=hide)
        vcol = torch.as_tensor(colors).to(verts.device)[:, self.prim].contiguous()
        normals = vertex_normals(verts, self.faces_d, self.adjacency)
        return color_render(verts, self.faces_d, vcol, cam, size, normals=normals, transform=transform)


class _BodyScene:
    """A body, optionally standing on the floor, as one mesh with one face list for the whole batch."""

    def __init__(self, body_faces, n_body_verts, device, floor=None):
        self.V = int(n_body_verts)
        bf = np.asarray(body_faces).astype(np.int32).reshape(-1, 3)
        self.floor_v = self.floor_c = None
        self.n_body_faces = len(bf)
        if floor is not None:
            fv, ff, fc = floor
            bf = np.concatenate([bf, ff + self.V]).astype(np.int32)
            self.floor_v, self.floor_c = torch.from_numpy(fv).to(device), torch.from_numpy(fc).to(device)
        self.faces = torch.from_numpy(bf).to(device)
        self.adjacency = vertex_adjacency(bf, self.V + (0 if floor is None else len(floor[0])))

    def render(self, verts, colors, cam, size, transform, with_body_mask=False):
        """verts [T, V, 3]; colors uint8 [T, 4] (one material per frame) or [T or 1, V, 4] (per vertex) -> rgba [T, H, W, 4];
        with_body_mask: (rgba, bool [T, H, W], true where the body -- not the floor -- is what the pixel shows)."""
        T = verts.shape[0]
        colors = torch.as_tensor(colors).to(verts.device)
        if colors.dim() == 2:
            colors = colors[:, None, :].expand(T, self.V, 4)
        colors = colors.expand(T, self.V, 4)
        if self.floor_v is not None:
            verts = torch.cat([verts, self.floor_v[None].expand(T, -1, -1)], dim=1)
            colors = torch.cat([colors, self.floor_c[None].expand(T, -1, -1)], dim=1)
        verts, colors = verts.contiguous(), colors.contiguous()
        normals = vertex_normals(verts, self.faces, self.adjacency)
        if not with_body_mask:
            return color_render(verts, self.faces, colors, cam, size, normals=normals, transform=transform)
        rgba, _, face = color_render(verts, self.faces, colors, cam, size, normals=normals, transform=transform, with_face_id=True)
        return rgba, (face >= 0) & (face < self.n_body_faces)


def lower_body_vertices(vert_segmentation):
    """The script's lower-body vertex list from data/smplx_vert_segmentation.json (a path or the loaded dict)."""
    if isinstance(vert_segmentation, (str, os.PathLike)):
        import json
        with open(vert_segmentation) as f:
            vert_segmentation = json.load(f)
    return sorted({int(i) for part in LOWER_BODY_PARTS for i in vert_segmentation[part]})


def _clip_verts(saved_data, key, bs, body_model, device):
    from .data_loaders.motion_representation import recover_from_repr_smpl
    names, dims = saved_data['repr_name_list'], saved_data['repr_dim_dict']
    x = torch.as_tensor(np.asarray(saved_data[key][bs:bs + 1], dtype=np.float32)).to(device)
    d, o = {}, 0
    for n in names:
        d[n] = x[..., o:o + dims[n]]
        o += dims[n]
    _, verts = recover_from_repr_smpl(d, recover_mode='smplx_params', smplx_model=body_model, return_verts=True)
    return verts[0]


def render_amass(saved_data, body_model, mask_scheme='lower', traj_mask_ratio=0.0, out_dir=None, interval=100, size=AMASS_SIZE,
                 vert_segmentation=None, device='cuda:0', return_images=False, skeleton_detail=(3, 32)):
    """eval_amass_full.py:286-395: for every `interval`-th clip of the driver's pickle, per frame, the predicted body (with its
    skeleton, occluded joints and foot contacts coloured), the input body (with the visible part of its skeleton) and the
    ground-truth-coloured body (the script feeds it the predicted vertices, :337), each on the checkerboard floor, flipped
    left-right.  Writes <out_dir>/{pred,input,gt}/seq_%03d/frame_%03d.png when `out_dir` is given; with `return_images`
    returns {'pred' | 'input' | 'gt': {clip: uint8 [T, H, W, 4] numpy}, 'body_mask' | 'skeleton_mask': {clip: bool [T, H, W]}}
    (where the predicted picture shows the body, and where its skeleton).  All frames of a clip are one batched call per
    scene.  `vert_segmentation`: the script's data/smplx_vert_segmentation.json; the input body's lower-body vertices get
    alpha 0.1 under 'lower' when it is given, none do otherwise."""
    if mask_scheme not in ('lower', 'full'):
        raise ValueError(f'unknown mask_scheme {mask_scheme!r}')
    faces = getattr(body_model, 'faces', None)
    if faces is None:
        raise _lib.RohmHipError('render_amass needs the body model\'s faces (SMPLXLayer.from_npz keeps them)')
    dev = torch.device(device)
    sx, sy = size[0] / AMASS_SIZE[0], size[1] / AMASS_SIZE[1]          # a smaller picture shows the same view
    cam = (AMASS_CAM[0] * sx, AMASS_CAM[1] * sy, AMASS_CAM[2] * sx, AMASS_CAM[3] * sy)
    to_cam = np.linalg.inv(np.asarray(AMASS_CAM_TRANS, dtype=np.float64))
    joints_rec = np.asarray(saved_data['rec_ric_data_rec_list_from_smpl'], dtype=np.float32)
    noisy = 'rec_ric_data_noisy_list' in saved_data
    joints_in = np.asarray(saved_data['rec_ric_data_noisy_list' if noisy else 'rec_ric_data_clean_list'], dtype=np.float32)
    repr_in = 'motion_repr_noisy_list' if noisy else 'motion_repr_clean_list'
    contact = np.asarray(saved_data['motion_repr_rec_list'])[:, :, -4:] > 0.5
    n_seq, T = joints_rec.shape[:2]
    start = end = 0
    mask_ids = None
    if mask_scheme == 'lower':
        mask_ids = list(LOWER_MASK_JOINTS)
    else:
        start = FULL_MASK_START
        end = start + int(traj_mask_ratio * CLIP_LEN_AMASS)
    t = np.arange(T)
    in_window = (t >= start) & (t < end)
    M = {k: np.asarray(v, dtype=np.uint8) for k, v in MATERIALS.items()}
    skel = SkeletonTemplate(dev, *skeleton_detail)
    scene = None
    images = {'pred': {}, 'input': {}, 'gt': {}, 'body_mask': {}, 'skeleton_mask': {}}
    for bs in range(0, n_seq, int(interval)):
        v_rec = _clip_verts(saved_data, 'motion_repr_rec_list', bs, body_model, dev)
        v_in = _clip_verts(saved_data, repr_in, bs, body_model, dev)
        V = v_rec.shape[1]
        if scene is None:
            scene = _BodyScene(faces, V, dev, floor=floor_mesh())
        col_rec = np.where(in_window[:, None], M['body_rec_occ'], M['body_rec_vis'])
        col_in = np.tile(M['body_noisy'], (1, V, 1))
        if mask_scheme == 'lower' and vert_segmentation is not None:
            col_in[0, lower_body_vertices(vert_segmentation), 3] = 26       # alpha 0.1 as trimesh stores it: round(25.5)
        j_rec, j_in = torch.from_numpy(joints_rec[bs]).to(dev), torch.from_numpy(joints_in[bs]).to(dev)
        c_rec, h_rec = skeleton_colors(T, mask_scheme, mask_ids, True, start, end, True, contact[bs])
        c_in, h_in = skeleton_colors(T, mask_scheme, mask_ids, False, start, end, False)
        window = torch.from_numpy(in_window).to(dev) if (mask_scheme == 'full' and in_window.any()) else None

        def finish(body, bones, dim_window):
            """render_img on both pictures (alpha 0.5 inside the 'full' window for the input), Image.paste, the flip"""
            out = requantize(body, 1.0)
            bones = None if bones is None else requantize(bones, 1.0)
            if dim_window and window is not None:
                out[window] = requantize(body[window], 0.5)
                bones[window] = requantize(bones[window], 0.5)
            if bones is not None:
                out = paste(out, bones)
            return flip_lr(out)
        body_rec = scene.render(v_rec, col_rec, cam, size, to_cam, with_body_mask=return_images)
        bones_rec = skel.render(j_rec, c_rec, h_rec, cam, size, to_cam)
        if return_images:
            body_rec, mask = body_rec
            images['body_mask'][bs] = mask.flip(-1).cpu().numpy()
            images['skeleton_mask'][bs] = (bones_rec[..., 3] > 0).flip(-1).cpu().numpy()
        clip = {
            'pred': finish(body_rec, bones_rec, False),
            'input': finish(scene.render(v_in, col_in, cam, size, to_cam), skel.render(j_in, c_in, h_in, cam, size, to_cam), True),
            'gt': finish(scene.render(v_rec, np.tile(M['body_gt'], (T, 1)), cam, size, to_cam), None, False),
        }
        for name, img in clip.items():
            host = img.cpu().numpy()
            if out_dir is not None:
                d = os.path.join(out_dir, name, 'seq_{}'.format(format(bs, '03d')))
                os.makedirs(d, exist_ok=True)
                for k in range(T):
                    write_png(os.path.join(d, 'frame_{}.png'.format(format(k, '03d'))), host[k])
            if return_images:
                images[name][bs] = host
    return images if return_images else None


def render_scene_clips(verts_rec, verts_input, joints_rec, faces, cam2world, f, c, mask_joint_vis=None, contact_lbl=None,
                       trans_scene2cano=None, size=(1920, 1080), background=None, skeleton_detail=(3, 32)):
    """The PROX / EgoBody pictures of eval_prox_egobody.py:415-443 for clips of T frames: the predicted body at alpha 0.9 and
    its skeleton (occluded joints from `mask_joint_vis` [n, T, 22], 1 = visible; contacts from `contact_lbl` [n, T, 4]) pasted
    over the background, and the input body overlaid on the same background.  verts_* [n, T, V, 3], joints_rec [n, T, 22, 3]
    device tensors, in scene coordinates, or in canonical ones with `trans_scene2cano` [n, 4, 4] (undone inside the
    renderer's transform); `cam2world` 4 x 4; f, c: the colour camera's focal lengths and centre (calibration Color.json);
    `background` uint8 [n, T, H, W, 3] device tensor, already undistorted, or None for black.
    -> (mesh_skel [n, T, H, W, 3], input [n, T, H, W, 3]) uint8 device tensors."""
    _lib.require_hip(verts_rec, verts_input, joints_rec)
    dev = verts_rec.device
    n, T, V = verts_rec.shape[:3]
    W, H = int(size[0]), int(size[1])
    cam = (float(f[0]), float(f[1]), float(c[0]), float(c[1]))
    to_cam = np.linalg.inv(np.asarray(cam2world, dtype=np.float64))
    scene = _BodyScene(faces, V, dev)
    skel = SkeletonTemplate(dev, *skeleton_detail)
    M = {k: np.asarray(v, dtype=np.uint8) for k, v in MATERIALS.items()}
    out_rec = torch.empty(n, T, H, W, 3, dtype=torch.uint8, device=dev)
    out_in = torch.empty_like(out_rec)
    for i in range(n):
        m = to_cam if trans_scene2cano is None else to_cam @ np.linalg.inv(
            np.asarray(trans_scene2cano[i].detach().cpu() if torch.is_tensor(trans_scene2cano) else trans_scene2cano[i], dtype=np.float64))
        bg = torch.zeros(T, H, W, 3, dtype=torch.uint8, device=dev) if background is None else _u8(background[i], (3,))
        occluded = None if mask_joint_vis is None else (np.asarray(
            mask_joint_vis[i].detach().cpu() if torch.is_tensor(mask_joint_vis) else mask_joint_vis[i]) == 0)
        lbl = None if contact_lbl is None else np.asarray(contact_lbl[i].detach().cpu() if torch.is_tensor(contact_lbl) else contact_lbl[i])
        col, hide = skeleton_colors(T, 'video', occluded, True, add_contact=lbl is not None, contact_lbl=lbl)
        body = requantize(scene.render(verts_rec[i], np.tile(M['body_rec_vis'], (T, 1)), cam, (W, H), m), 0.9)
        bones = requantize(skel.render(joints_rec[i].float(), col, hide, cam, (W, H), m), 1.0)
        out_rec[i] = paste(paste(bg, body), bones)
        out_in[i] = overlay(bg, scene.render(verts_input[i], np.tile(M['body_noisy'], (T, 1)), cam, (W, H), m))
    return out_rec, out_in
