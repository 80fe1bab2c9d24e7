"""CPU checks of the float64 restatement (tests/raster_ref.py) against closed forms, and of the PLY reader of
rohm_amd.occlusion on files written here."""
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raster_ref as rr  # noqa: E402

CAM = (106.053, 106.038, 95.13, 53.677)          # the script's intrinsics at a tenth of the size
SIZE = (192, 108)


def _rays(cam=CAM, size=SIZE):
    fx, fy, cx, cy = cam
    x, y = np.meshgrid(np.arange(size[0]), np.arange(size[1]), indexing='xy')
    return np.stack([(x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy, np.ones(x.shape)], -1)


def test_sphere_matches_analytic_depth():
    c, r = np.array([0.1, -0.05, 3.0]), 0.5
    v, f = rr.uv_sphere(64, 128, r, c)
    img, edge = rr.render(v, f, CAM, SIZE, with_edges=True)
    d = _rays()
    dc, dd = d @ c, (d * d).sum(-1)
    disc = dc * dc - dd * (c @ c - r * r)
    z = (dc - np.sqrt(np.maximum(disc, 0))) / dd
    # the faceted sphere lies inside the analytic one by at most r (1 - cos(pi / 128)) ~ 1.5e-4 along the normal; stay
    # away from the silhouette, where that turns into a large depth difference
    inner = disc > 0.5 * dd * r * r
    assert inner.sum() > 300
    assert (img[inner] > 0).all()
    assert np.abs(img[inner] - z[inner]).max() < 1e-3
    assert (img[disc < -1e-2 * dd * r * r] == 0).all()
    assert np.isfinite(edge[inner]).all() and (edge[inner] >= 0).all()


def test_tilted_plane_is_exact():
    n, k = np.array([0.3, -0.2, 1.0]), 4.0                 # plane n . p = k
    corners = [(-9, -9), (9, -9), (9, 9), (-9, 9)]
    v, f = rr.quad(*[(x, y, (k - n[0] * x - n[1] * y) / n[2]) for x, y in corners])
    img = rr.render(v, f, CAM, SIZE)
    z = k / (_rays() @ n)
    assert (img > 0).all()
    # the float32 vertices are the input; the plane through them differs from the ideal one by their rounding
    assert np.abs(img - z).max() < 5e-6
    # two-sided by default, a culled back face disappears; the winding above faces the camera
    assert (rr.render(v, f[:, ::-1], CAM, SIZE) > 0).all()
    front = rr.render(v, f, CAM, SIZE, cull_backfaces=True)
    back = rr.render(v, f[:, ::-1], CAM, SIZE, cull_backfaces=True)
    assert ((front > 0).all() and (back == 0).all()) or ((front == 0).all() and (back > 0).all())
    nrm = np.cross(v[1] - v[0], v[2] - v[0])
    assert ((front > 0).all()) == bool(nrm @ v[0] < 0)


def test_triangle_across_the_camera_plane():
    # a floor triangle 0.5 m below the camera from z = -2 (behind it) to z = +6
    tri = np.array([[-1.5, 0.5, -2.0], [1.5, 0.5, -2.0], [0.2, 0.5, 6.0]], dtype=np.float32)
    img, edge = rr.render(tri, np.array([[0, 1, 2]], dtype=np.int32), CAM, SIZE, with_edges=True)
    d = _rays()
    with np.errstate(divide='ignore'):
        z = 0.5 / d[..., 1]
    hitp = d * z[..., None]
    # inside test in the plane y = 0.5, on (x, z)
    a, b, c = tri[:, [0, 2]].astype(np.float64)
    q = hitp[..., [0, 2]]

    def side(p0, p1):
        return (p1[0] - p0[0]) * (q[..., 1] - p0[1]) - (p1[1] - p0[1]) * (q[..., 0] - p0[0])
    s0, s1, s2 = side(a, b), side(b, c), side(c, a)
    inside = ((s0 >= 0) & (s1 >= 0) & (s2 >= 0)) | ((s0 <= 0) & (s1 <= 0) & (s2 <= 0))
    expect = inside & (d[..., 1] > 0) & (z >= rr.ZNEAR) & (z <= rr.ZFAR)
    clear = edge > 1e-6
    assert expect.sum() > 200
    assert ((img > 0) == expect)[clear].all()
    assert np.abs(img - z)[expect & clear].max() < 1e-9
    # the near plane cuts it: nothing closer than znear, and a triangle wholly behind the camera draws nothing
    assert img[img > 0].min() >= rr.ZNEAR
    assert (rr.render(tri * np.array([1, 1, -1], np.float32) - np.array([0, 0, 7], np.float32),
                      np.array([[0, 1, 2]], dtype=np.int32), CAM, SIZE) == 0).all()


def test_edge_distance_of_a_single_triangle():
    tri = np.array([[-0.5, -0.4, 2.0], [0.6, -0.3, 2.0], [0.0, 0.5, 2.0]], dtype=np.float32)
    img, edge = rr.render(tri, np.array([[0, 1, 2]], dtype=np.int32), CAM, SIZE, with_edges=True)
    fx, fy, cx, cy = CAM
    t64 = tri.astype(np.float64)
    uv = np.stack([t64[:, 0] / t64[:, 2] * fx + cx, t64[:, 1] / t64[:, 2] * fy + cy], -1)
    x, y = np.meshgrid(np.arange(SIZE[0]) + 0.5, np.arange(SIZE[1]) + 0.5, indexing='xy')
    best = np.full(x.shape, np.inf)
    for i in range(3):
        p0, p1 = uv[i], uv[(i + 1) % 3]
        e = p1 - p0
        t = np.clip(((x - p0[0]) * e[0] + (y - p0[1]) * e[1]) / (e @ e), 0, 1)
        best = np.minimum(best, np.hypot(x - (p0[0] + t * e[0]), y - (p0[1] + t * e[1])))
    hit = img > 0
    assert hit.sum() > 1000
    assert np.abs(edge[hit] - best[hit]).max() < 1e-9              # inside: exactly the distance to the outline
    near = np.isfinite(edge) & ~hit
    assert (edge[near] <= best[near] + 1e-9).all()                 # outside: a lower bound


def test_distortion_round_trip_and_projection():
    g = np.random.Generator(np.random.PCG64(3))
    dist = [-0.12, 0.09, 0.0012, -0.0007, -0.02]
    xy = g.uniform(-0.6, 0.6, size=(500, 2))
    assert np.abs(rr.undistort(rr.distort(xy, dist), dist) - xy).max() < 1e-12
    assert np.array_equal(rr.distort(xy, [0, 0, 0, 0, 0]), xy)
    # pure radial distortion keeps the direction, barrel (k1 < 0) pulls inwards
    rad = rr.distort(xy, [-0.1, 0, 0, 0, 0])
    assert np.abs(rad[:, 0] * xy[:, 1] - rad[:, 1] * xy[:, 0]).max() < 1e-15
    assert (np.hypot(*rad.T) <= np.hypot(*xy.T)).all()
    K = [[1060.53, 0, 951.30], [0, 1060.38, 536.77], [0, 0, 1]]
    pts = np.array([[0.0, 0.0, 2.0], [0.5, -0.25, 2.0], [-3.0, 0.1, 1.0]])
    uv = rr.project(pts, K, [0, 0, 0, 0, 0])
    assert np.allclose(uv, [[951.30, 536.77], [951.30 + 1060.53 * 0.25, 536.77 - 1060.38 * 0.125], [951.30 - 3181.59, 536.77 + 106.038]])
    assert rr.to_pixels(np.array([-0.7, 0.7, 12.9, -3.2])).tolist() == [0, 0, 12, -3]      # astype(int) truncates toward zero


def test_mask_decision():
    scene = np.zeros((4, 6))
    scene[1, 2], scene[2, 3] = 2.0, 2.0
    pix = np.array([[[2, 1], [3, 2], [0, 0], [-1, 2], [6, 1], [2, 1]]])
    body = np.array([[2.2, 2.05, 5.0, 9.0, 9.0, 0.0]])
    mask, margin = rr.occlusion_mask(pix, scene, body)
    #            behind      within thr  scene == 0  outside  outside  body missed
    assert mask.tolist() == [[0.0, 1.0, 1.0, 1.0, 1.0, 1.0]]
    assert margin[0, 0] == pytest.approx(0.1) and margin[0, 1] == pytest.approx(-0.05)


# ---- the PLY reader (new with rohm_amd.occlusion) -----------------------------------------------------------------------
def _mesh():
    v = np.array([[0, 0, 0], [1, 0, 0.5], [1, 1, 1], [0, 1, 0.25], [0.5, 0.5, 2]], dtype=np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3], [1, 4, 2]], dtype=np.int32)
    return v, f


def test_ply_ascii_with_extra_properties_and_a_quad(tmp_path):
    from rohm_amd.occlusion import read_ply
    v, f = _mesh()
    lines = ['ply', 'format ascii 1.0', 'comment made by a test', f'element vertex {len(v)}', 'property float x',
             'property float y', 'property float z', 'property uchar red', 'property uchar green', 'property uchar blue',
             'element face 3', 'property list uchar int vertex_indices', 'end_header']
    lines += [f'{p[0]} {p[1]} {p[2]} 10 20 30' for p in v.tolist()]
    lines += ['4 0 1 2 3', '3 1 4 2', '3 0 2 3']
    path = tmp_path / 'a.ply'
    path.write_text('\n'.join(lines) + '\n')
    rv, rf = read_ply(str(path))
    assert rv.dtype == np.float32 and rf.dtype == np.int32
    assert np.array_equal(rv, v)
    assert rf.tolist() == [[0, 1, 2], [0, 2, 3], [1, 4, 2], [0, 2, 3]]


@pytest.mark.parametrize('index_type', ['int', 'uint'])
def test_ply_binary_little_endian(tmp_path, index_type):
    from rohm_amd.occlusion import read_ply
    v, f = _mesh()
    head = ['ply', 'format binary_little_endian 1.0', f'element vertex {len(v)}', 'property float x', 'property float y',
            'property float z', 'property float nx', 'property float ny', 'property float nz', 'property uchar red',
            'property uchar green', 'property uchar blue', 'property uchar alpha', f'element face {len(f)}',
            f'property list uchar {index_type} vertex_indices', 'end_header']
    blob = ('\n'.join(head) + '\n').encode()
    for p in v.tolist():
        blob += struct.pack('<6f4B', p[0], p[1], p[2], 0.0, 0.0, 1.0, 1, 2, 3, 255)
    for t in f.tolist():
        blob += struct.pack('<B3' + ('i' if index_type == 'int' else 'I'), 3, *t)
    path = tmp_path / 'b.ply'
    path.write_bytes(blob)
    rv, rf = read_ply(str(path))
    assert np.array_equal(rv, v) and np.array_equal(rf, f)
    assert rv.dtype == np.float32 and rf.dtype == np.int32


def test_ply_binary_mixed_polygons_and_rejects(tmp_path):
    from rohm_amd.occlusion import read_ply
    v, _ = _mesh()
    head = ['ply', 'format binary_little_endian 1.0', f'element vertex {len(v)}', 'property double x', 'property double y',
            'property double z', 'element face 2', 'property list uchar int vertex_indices', 'end_header']
    blob = ('\n'.join(head) + '\n').encode()
    for p in v.tolist():
        blob += struct.pack('<3d', *p)
    blob += struct.pack('<B4i', 4, 0, 1, 2, 3) + struct.pack('<B3i', 3, 1, 4, 2)
    path = tmp_path / 'c.ply'
    path.write_bytes(blob)
    rv, rf = read_ply(str(path))
    assert np.array_equal(rv, v)
    assert rf.tolist() == [[0, 1, 2], [0, 2, 3], [1, 4, 2]]
    bad = tmp_path / 'd.ply'
    bad.write_bytes(b'ply\nformat binary_big_endian 1.0\nelement vertex 0\nend_header\n')
    with pytest.raises(ValueError):
        read_ply(str(bad))
    with pytest.raises(ValueError):
        (tmp_path / 'e.ply').write_bytes(b'not a ply')
        read_ply(str(tmp_path / 'e.ply'))
