"""TEST INFRASTRUCTURE ONLY: float64 numpy restatement of the shading rule of csrc/shade.hip (stated in include/rohm_hip.h),
of its vertex normals and skeleton mesh, and of the scripts' image arithmetic.  It does not import rohm_amd.

The rule: coverage and depth as in raster_ref; the winner of a pixel is the smallest float32 depth and, among equal ones,
the smallest face index; weights are the barycentrics of the hit point (here from the Moeller-Trumbore test; the device
takes them from its homogeneous edge functions: a different formulation of the same thing); n = normalise(sum l_i n_i) or
the face normal, turned toward the eye unless back faces are culled; lambert = max(0, -n_z);
out_k = floor(255 min(1, c_k (ambient + diffuse lambert)) + 0.5), out_a = floor(255 a + 0.5).
"""
import math

import numpy as np

import raster_ref as rr

AMBIENT, DIFFUSE = 0.3, 3.0 / math.pi
LIMBS = ((15, 12), (12, 13), (13, 16), (16, 18), (18, 20), (12, 14), (14, 17), (17, 19), (19, 21), (12, 9), (9, 6), (6, 3), (3, 0),
         (0, 1), (1, 4), (4, 7), (7, 10), (0, 2), (2, 5), (5, 8), (8, 11))


def _unit(v):
    n = np.linalg.norm(v, axis=-1, keepdims=True)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(n > 0, v / n, 0.0)


def vertex_normals(verts, faces):
    """Area-weighted smooth normals [V, 3] float64; (0, 0, 0) for a vertex without a face or with a zero sum."""
    v = np.asarray(verts, dtype=np.float64)
    f = np.asarray(faces)
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    acc = np.zeros_like(v)
    for k in range(3):
        np.add.at(acc, f[:, k], fn)
    return _unit(acc)


def render(verts, faces, colors, normals=None, cam=rr.PROX_CAM, size=rr.PROX_SIZE, ambient=AMBIENT, diffuse=DIFFUSE,
           cull_backfaces=False, znear=rr.ZNEAR, zfar=rr.ZFAR):
    """-> dict: rgba uint8 [H, W, 4], depth float64 [H, W] (0 = miss), face_id int64 [H, W] (-1 = miss), gap float64 [H, W]
    (distance in depth from the winner to the next hit along the ray, inf if there is none), weights float64 [H, W, 3].
    verts [V, 3] in camera space, colors uint8 [V, 4], normals [V, 3] or None (flat)."""
    fx, fy, cx, cy = cam
    W, H = size
    faces = np.asarray(faces)
    p = np.asarray(verts, dtype=np.float64)[faces]
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    fnrm = np.cross(e1, e2)
    keep = np.linalg.norm(fnrm, axis=1) > 0
    if cull_backfaces:
        keep &= (fnrm * p[:, 0]).sum(1) < 0
    bounds = rr._bounds(p, cam, size, znear)
    bounds[~keep] = (0, 0, -1, -1)
    hits = []
    for idx, Sw, Sh in rr._blocks(bounds):
        x, y, ok = rr._grid(bounds, idx, Sw, Sh, size)
        d = np.stack([(x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy, np.ones(ok.shape)], -1)
        E1, E2, V0 = (a[idx][:, None, None, :] for a in (e1, e2, p[:, 0]))
        P = np.cross(d, E2)
        det = (E1 * P).sum(-1)
        with np.errstate(divide='ignore', invalid='ignore'):
            inv = 1.0 / det
            T = -V0
            bu = (T * P).sum(-1) * inv
            Q = np.cross(np.broadcast_to(T, d.shape), E1)
            bv = (d * Q).sum(-1) * inv
            t = (E2 * Q).sum(-1) * inv
            hit = ok & (det != 0) & (bu >= 0) & (bv >= 0) & (bu + bv <= 1) & (t >= znear) & (t <= zfar)
        if hit.any():
            face = np.broadcast_to(idx[:, None, None], hit.shape)
            hits.append(np.stack([(y * W + x)[hit], face[hit]], 0).astype(np.int64))
            hits.append(np.stack([t[hit], bu[hit], bv[hit]], 0))
    out = {'rgba': np.zeros((H, W, 4), np.uint8), 'depth': np.zeros((H, W)), 'face_id': np.full((H, W), -1, np.int64),
           'gap': np.full((H, W), np.inf), 'weights': np.zeros((H, W, 3))}
    if not hits:
        return out
    ints, flts = np.concatenate(hits[0::2], 1), np.concatenate(hits[1::2], 1)
    pix, face = ints
    t, bu, bv = flts
    order = np.lexsort((face, t.astype(np.float32), pix))          # by pixel, then float32 depth, then face index
    pix, face, t, bu, bv = pix[order], face[order], t[order], bu[order], bv[order]
    first = np.concatenate([[True], pix[1:] != pix[:-1]])
    nxt = np.concatenate([~first[1:], [False]])          # followed by another hit of the same pixel
    w = np.nonzero(first)[0]
    gap = np.where(nxt[w], t[np.minimum(w + 1, len(t) - 1)] - t[w], np.inf)
    wp, wf = pix[w], face[w]
    lam = np.stack([1.0 - bu[w] - bv[w], bu[w], bv[w]], -1)
    if normals is None:
        n = _unit(fnrm[wf])
    else:
        n = _unit((np.asarray(normals, dtype=np.float64)[faces[wf]] * lam[..., None]).sum(1))
    yy, xx = wp // W, wp % W
    d = np.stack([(xx + 0.5 - cx) / fx, (yy + 0.5 - cy) / fy, np.ones(len(wp))], -1)
    if not cull_backfaces:
        n = np.where(((n * d).sum(-1) > 0)[:, None], -n, n)
    shade = ambient + diffuse * np.maximum(0.0, -n[:, 2])
    C = (np.asarray(colors, dtype=np.float64)[faces[wf]] * lam[..., None]).sum(1) / 255.0
    rgb = np.floor(255.0 * np.minimum(1.0, C[:, :3] * shade[:, None]) + 0.5)
    a = np.floor(255.0 * C[:, 3] + 0.5)
    out['rgba'].reshape(-1, 4)[wp] = np.clip(np.concatenate([rgb, a[:, None]], 1), 0, 255).astype(np.uint8)
    out['depth'].reshape(-1)[wp] = t[w]
    out['face_id'].reshape(-1)[wp] = wf
    out['gap'].reshape(-1)[wp] = gap
    out['weights'].reshape(-1, 3)[wp] = lam
    return out


def skeleton_mesh(joints, sphere, cyl, limbs=LIMBS, hide=None, r_joint=0.025, r_limb=0.01):
    """joints [N, J, 3] -> verts [N, J Vs + L Vc, 3] float64 by the rule of rohm_hip.h (float32 frame decisions are not
    restated: the axis choice is made on float64 values)."""
    j = np.asarray(joints, dtype=np.float64)
    s, c = np.asarray(sphere, dtype=np.float64), np.asarray(cyl, dtype=np.float64)
    N, J = j.shape[:2]
    L = len(limbs)
    hide = np.zeros((N, J + L), bool) if hide is None else np.asarray(hide).astype(bool)
    out = []
    for n in range(N):
        parts = []
        for k in range(J):
            parts.append(j[n, k] + (0.0 if hide[n, k] else r_joint) * s)
        for l, (a_, b_) in enumerate(limbs):
            p1, p2 = j[n, a_], j[n, b_]
            ln = np.linalg.norm(p2 - p1)
            if hide[n, J + l] or ln == 0:
                parts.append(np.tile(p1, (len(c), 1)))
                continue
            a = (p2 - p1) / ln
            e = np.zeros(3)
            e[int(np.argmin(np.abs(a)))] = 1.0
            u = np.cross(a, e)
            u /= np.linalg.norm(u)
            w = np.cross(a, u)
            parts.append(p1 + r_limb * (c[:, :1] * u + c[:, 1:2] * w) + ln * c[:, 2:3] * a)
        out.append(np.concatenate(parts))
    return np.stack(out)


# ---- image arithmetic (integer / float32 numpy) ----------------------------------------------------------------------
def requantize(rgba, alpha):
    x = rgba.astype(np.float32) / np.float32(255.0)
    x[..., -1] = x[..., -1] * np.float32(alpha)
    return (x * np.float32(255)).astype(np.uint8)


def paste(dst, src_rgba):
    a = src_rgba[..., 3:4].astype(np.int64)
    s = src_rgba[..., :dst.shape[-1]].astype(np.int64)
    t = s * a + dst.astype(np.int64) * (255 - a) + 128
    return ((t + (t >> 8)) >> 8).astype(np.uint8)


def overlay(dst_rgb, src_rgba):
    return np.where(src_rgba[..., 3:4] > 0, src_rgba[..., :3], dst_rgb).astype(np.uint8)


def flip_lr(img):
    return np.ascontiguousarray(img[..., ::-1, :])
