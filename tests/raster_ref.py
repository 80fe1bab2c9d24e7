"""TEST INFRASTRUCTURE ONLY: float64 numpy restatement of the depth-rendering rule of csrc/raster.hip and of the mask
decision of utils/get_occlusion_mask.py:131-143.  It does not import rohm_amd.

The rule: a pinhole camera in OpenCV axes (x right, y down, z forward); pixel (x, y) samples the ray through
u = x + 0.5, v = y + 0.5, direction d = ((u - cx) / fx, (v - cy) / fy, 1); the depth is the smallest z in [znear, zfar]
at which the ray meets any triangle (both sides), 0 where it meets none.

`render` intersects rays and triangles with the Moeller-Trumbore test (the device uses homogeneous edge functions: a
different formulation of the same rule).  `edge_distance` returns, per pixel, how far the sample lies from the nearest
edge of any triangle whose bounds contain it -- the pixels where two correct implementations may disagree on hit / miss
are those within rounding distance of an edge.  The pyrender / OpenCV tools themselves are not available where this
project is built, so nothing here is pinned to them; `distort` is OpenCV's published model.
"""
import numpy as np

ZNEAR, ZFAR = 0.05, 100.0
PROX_CAM = (1060.53, 1060.38, 951.30, 536.77)      # get_occlusion_mask.py:64-69
PROX_SIZE = (1920, 1080)


# ---- meshes ---------------------------------------------------------------------------------------------------------
def uv_sphere(n_lat=64, n_lon=128, radius=0.5, center=(0.0, 0.0, 3.0)):
    """(n_lat + 1) x n_lon vertices, 2 n_lat n_lon faces (those at the poles are degenerate and never hit)."""
    th = np.linspace(0.0, np.pi, n_lat + 1)[:, None]
    ph = (np.arange(n_lon) * (2 * np.pi / n_lon))[None, :]
    v = np.stack([np.sin(th) * np.cos(ph), np.cos(th) * np.ones_like(ph), np.sin(th) * np.sin(ph)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(n_lat), np.arange(n_lon), indexing='ij')
    a, b = i * n_lon + j, i * n_lon + (j + 1) % n_lon
    c, d = a + n_lon, b + n_lon
    f = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([b, d, c], -1).reshape(-1, 3)])
    return (v * radius + np.asarray(center)).astype(np.float32), f.astype(np.int32)


def height_field(n=200, z0=4.0, half=(2.6, 1.6), amp=0.15, seed=0):
    """n x n vertices over [-half, half], z = z0 + smooth bumps + a little noise; 2 (n - 1)^2 faces."""
    g = np.random.Generator(np.random.PCG64(seed))
    x, y = np.meshgrid(np.linspace(-half[0], half[0], n), np.linspace(-half[1], half[1], n), indexing='xy')
    z = z0 + amp * np.sin(3.1 * x + 0.4) * np.cos(2.3 * y - 0.2) + 0.01 * g.standard_normal((n, n))
    x = x + 0.002 * g.standard_normal((n, n))
    y = y + 0.002 * g.standard_normal((n, n))
    v = np.stack([x, y, z], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing='ij')
    a = i * n + j
    f = np.concatenate([np.stack([a, a + 1, a + n], -1).reshape(-1, 3), np.stack([a + 1, a + n + 1, a + n], -1).reshape(-1, 3)])
    return v.astype(np.float32), f.astype(np.int32)


def box(center=(0.3, -0.2, 1.0), half=(3.0, 2.0, 5.0)):
    """A box around the camera: 12 faces, some behind it, some across z = 0 and the near plane."""
    s = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=np.float64)
    v = s * np.asarray(half) + np.asarray(center)
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = [t for a, b, c, d in q for t in ((a, b, c), (a, c, d))]
    return v.astype(np.float32), np.asarray(f, dtype=np.int32)


def quad(p0, p1, p2, p3):
    return np.asarray([p0, p1, p2, p3], dtype=np.float32), np.asarray([[0, 1, 2], [0, 2, 3]], dtype=np.int32)


def merge(*meshes):
    vs, fs, off = [], [], 0
    for v, f in meshes:
        vs.append(v)
        fs.append(f + off)
        off += len(v)
    return np.concatenate(vs).astype(np.float32), np.concatenate(fs).astype(np.int32)


# ---- rendering ------------------------------------------------------------------------------------------------------
def _bounds(p, cam, size, znear):
    """Inclusive pixel bounds per triangle ([F, 4] x0, y0, x1, y1; x1 < x0: nothing to draw).  A triangle with a vertex
    in front of the near plane and one behind it gets the whole image."""
    fx, fy, cx, cy = cam
    W, H = size
    z = p[:, :, 2]
    front = (z >= znear).all(1)
    behind = (z < znear).all(1)
    with np.errstate(divide='ignore', invalid='ignore'):
        u = p[:, :, 0] / z * fx + cx
        v = p[:, :, 1] / z * fy + cy
    b = np.empty((len(p), 4), np.int64)
    big = 1 << 40
    uc, vc = np.clip(np.nan_to_num(u, nan=0.0), -big, big), np.clip(np.nan_to_num(v, nan=0.0), -big, big)
    b[:, 0], b[:, 1] = np.floor(uc.min(1)) - 1, np.floor(vc.min(1)) - 1
    b[:, 2], b[:, 3] = np.floor(uc.max(1)) + 1, np.floor(vc.max(1)) + 1
    b[~front] = (0, 0, W - 1, H - 1)
    b[:, 0], b[:, 1] = np.maximum(b[:, 0], 0), np.maximum(b[:, 1], 0)
    b[:, 2], b[:, 3] = np.minimum(b[:, 2], W - 1), np.minimum(b[:, 3], H - 1)
    b[behind] = (0, 0, -1, -1)
    return b


def _blocks(bounds, max_cells=1 << 20):
    """Group triangles by padded bounds size: yields (indices, S) with S x S covering each triangle's bounds."""
    w, h = bounds[:, 2] - bounds[:, 0] + 1, bounds[:, 3] - bounds[:, 1] + 1
    side = np.maximum(w, h)
    live = (w > 0) & (h > 0)
    lo = 0
    for S in (4, 8, 16, 32, 64, 128):
        idx = np.nonzero(live & (side > lo) & (side <= S))[0]
        per = max(1, max_cells // (S * S))
        for k in range(0, len(idx), per):
            yield idx[k:k + per], S, S
        lo = S
    for i in np.nonzero(live & (side > lo))[0]:
        yield np.array([i]), int(w[i]), int(h[i])


def _grid(bounds, idx, Sw, Sh, size):
    x = bounds[idx, 0][:, None, None] + np.arange(Sw)[None, None, :]
    y = bounds[idx, 1][:, None, None] + np.arange(Sh)[None, :, None]
    ok = (x <= bounds[idx, 2][:, None, None]) & (y <= bounds[idx, 3][:, None, None])
    x, y = np.broadcast_to(x, ok.shape), np.broadcast_to(y, ok.shape)
    return x, y, ok


def render(verts, faces, cam=PROX_CAM, size=PROX_SIZE, znear=ZNEAR, zfar=ZFAR, cull_backfaces=False, with_edges=False):
    """Depth image [H, W] float64 (0 = nothing hit).  with_edges: also the per-pixel distance (pixels) from the sample
    to the nearest edge of any triangle whose bounds contain it (inf where there is none)."""
    fx, fy, cx, cy = cam
    W, H = size
    p = np.asarray(verts, dtype=np.float64)[np.asarray(faces)]          # [F, 3, 3]
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    nrm = np.cross(e1, e2)
    keep = np.linalg.norm(nrm, axis=1) > 0
    if cull_backfaces:
        keep &= (nrm * p[:, 0]).sum(1) < 0          # counter-clockwise as seen from the camera: normal toward the eye
    bounds = _bounds(p, cam, size, znear)
    bounds[~keep] = (0, 0, -1, -1)
    depth = np.full(H * W, np.inf)
    edge = np.full(H * W, np.inf)
    # homogeneous edge functions for the distance helper: e_i = (p_j x p_k) . d is affine in the pixel coordinates
    if with_edges:
        nn = np.stack([np.cross(p[:, 1], p[:, 2]), np.cross(p[:, 2], p[:, 0]), np.cross(p[:, 0], p[:, 1])], 1)   # [F, 3, 3]
        sg = np.sign((p[:, 0] * nn[:, 0]).sum(1))
    for idx, Sw, Sh in _blocks(bounds):
        x, y, ok = _grid(bounds, idx, Sw, Sh, size)
        d = np.stack([(x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy, np.ones(ok.shape)], -1)          # [n, Sh, Sw, 3]
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
        flat = (y * W + x)
        if hit.any():
            np.minimum.at(depth, flat[hit], t[hit])
        if with_edges:
            N = nn[idx] * sg[idx][:, None, None]                                                  # [n, 3, 3]
            e = np.einsum('nic,nyxc->nyxi', N, d)                                                 # [n, Sh, Sw, 3]
            gl = np.sqrt((N[:, :, 0] / fx) ** 2 + (N[:, :, 1] / fy) ** 2)                         # [n, 3]
            with np.errstate(divide='ignore', invalid='ignore'):
                dist = e / gl[:, None, None, :]
            dist = np.where(np.isfinite(dist), dist, np.inf)
            inside = (dist >= 0).all(-1)
            bd = np.where(inside, dist.min(-1), (-dist).max(-1))
            np.minimum.at(edge, flat[ok], np.abs(bd[ok]))
    img = np.where(np.isfinite(depth), depth, 0.0).reshape(H, W)
    return (img, edge.reshape(H, W)) if with_edges else img


def edge_distance(verts, faces, cam=PROX_CAM, size=PROX_SIZE, znear=ZNEAR):
    """Per pixel, the distance in pixels from the sample point to the nearest edge of any triangle overlapping it."""
    return render(verts, faces, cam, size, znear=znear, with_edges=True)[1]


# ---- projection and decision ------------------------------------------------------------------------------------------
def distort(xy, dist):
    """OpenCV's model on normalised coordinates [..., 2]: radial (k1, k2, k3) and tangential (p1, p2) terms."""
    k1, k2, p1, p2, k3 = (float(v) for v in dist)
    x, y = xy[..., 0], xy[..., 1]
    r2 = x * x + y * y
    radial = 1.0 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    xd = x * radial + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    yd = y * radial + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    return np.stack([xd, yd], -1)


def undistort(xy_d, dist, iters=50):
    """Inverse of `distort` by fixed-point iteration (for round-trip checks)."""
    k1, k2, p1, p2, k3 = (float(v) for v in dist)
    x, y = xy_d[..., 0].copy(), xy_d[..., 1].copy()
    for _ in range(iters):
        r2 = x * x + y * y
        radial = 1.0 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
        dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
        x, y = (xy_d[..., 0] - dx) / radial, (xy_d[..., 1] - dy) / radial
    return np.stack([x, y], -1)


def project(points, camera_mtx, dist):
    """cv2.projectPoints with zero rvec / tvec: [..., 3] -> continuous pixel coordinates [..., 2] (float64)."""
    pts = np.asarray(points, dtype=np.float64)
    K = np.asarray(camera_mtx, dtype=np.float64).reshape(3, 3)
    z = np.where(pts[..., 2] != 0, pts[..., 2], 1.0)
    xy = distort(pts[..., :2] / z[..., None], dist)
    return np.stack([xy[..., 0] * K[0, 0] + K[0, 2], xy[..., 1] * K[1, 1] + K[1, 2]], -1)


def to_pixels(uv):
    """numpy's astype(int) on finite values: truncation toward zero."""
    return np.trunc(uv).astype(np.int64)


def occlusion_mask(pixels, scene_depth, body_depth_at, thr=0.1):
    """get_occlusion_mask.py:138-143.  pixels [N, J, 2] ints, scene_depth [H, W], body_depth_at [N, J] (the body's depth
    at each joint's pixel; ignored outside the image) -> ([N, J] float64 mask, [N, J] margin body - scene - thr)."""
    H, W = scene_depth.shape
    x, y = pixels[..., 0], pixels[..., 1]
    inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
    s = np.where(inside, scene_depth[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)], 0.0)
    margin = body_depth_at - s - thr
    occluded = inside & (s != 0) & (margin > 0)
    return 1.0 - occluded.astype(np.float64), margin
