"""CPU: the shading restatement tests/shade_ref.py and the host builders of rohm_amd.render against closed forms.

pyrender does not exist where this project is built, so nothing is compared with it; the restatement is the reference of
tests/test_gpu_render.py and is itself checked here against values worked out by hand.
"""
import math
import struct
import zlib

import numpy as np
import pytest

import raster_ref as rr
import shade_ref as sr
from rohm_amd import render as R

CAM = tuple(v / 4 for v in rr.PROX_CAM)
SIZE = (480, 270)
W, H = SIZE


def _level(v):
    return math.floor(255.0 * min(1.0, v) + 0.5)


def _quad(z_top, z_bottom, color):
    """x in [-0.5, 0.5], y in [-0.4, 0.4]; depth runs linearly from z_top (y = -0.4) to z_bottom (y = 0.4)."""
    v, f = rr.quad((-0.5, -0.4, z_top), (0.5, -0.4, z_top), (0.5, 0.4, z_bottom), (-0.5, 0.4, z_bottom))
    return v, f, np.tile(np.asarray(color, np.uint8), (4, 1))


def test_fronto_parallel_quad_has_the_closed_form_colour():
    v, f, c = _quad(3.0, 3.0, (200, 100, 50, 255))
    out = sr.render(v, f, c, None, CAM, SIZE)
    hit = out['face_id'] >= 0
    assert hit.sum() > 5000
    want = [_level(k / 255.0 * (sr.AMBIENT + sr.DIFFUSE)) for k in (200, 100, 50)] + [255]
    assert (out['rgba'][hit] == np.asarray(want, np.uint8)).all()
    assert (out['rgba'][~hit] == 0).all()
    assert np.allclose(out['depth'][hit], 3.0, atol=1e-12)
    # smooth normals of a flat quad are the face normal: same picture
    again = sr.render(v, f, c, sr.vertex_normals(v, f), CAM, SIZE)
    assert (again['rgba'] == out['rgba']).all()


@pytest.mark.parametrize('flip', [False, True])
def test_tilted_quad_has_the_cosine_factor(flip):
    """Tilted about the x axis by atan(dz / dy): n = +-(0, -dz, dy) / |.|, so lambert = dy / hypot(dy, dz) on both sides."""
    z0, z1 = 2.6, 3.4
    v, f, c = _quad(z0, z1, (128, 128, 128, 200))
    if flip:
        f = f[:, ::-1].copy()
    out = sr.render(v, f, c, None, CAM, SIZE)
    hit = out['face_id'] >= 0
    assert hit.sum() > 5000
    cos = 0.8 / math.hypot(0.8, z1 - z0)
    assert abs(cos - math.cos(math.pi / 4)) < 1e-12
    k = _level(128 / 255.0 * (sr.AMBIENT + sr.DIFFUSE * cos))
    assert (out['rgba'][hit] == np.asarray([k, k, k, 200], np.uint8)).all()
    # culled: one winding is dropped, the other keeps its colour
    culled = sr.render(v, f, c, None, CAM, SIZE, cull_backfaces=True)
    front = (np.cross(v[f[0, 1]] - v[f[0, 0]], v[f[0, 2]] - v[f[0, 0]]) * v[f[0, 0]]).sum() < 0
    assert ((culled['face_id'] >= 0) == (hit & front)).all()


def test_triangle_weights_are_perspective_correct():
    """Red, green and blue corners at depths 2, 3 and 5.  A pixel with screen-space (affine) barycentrics b_i of the projected
    triangle has hit-point weights l_i = (b_i / z_i) / sum_j (b_j / z_j)."""
    fx, fy, cx, cy = CAM
    v = np.array([[-0.5, -0.4, 2.0], [0.9, -0.3, 3.0], [0.2, 1.2, 5.0]], dtype=np.float32)
    f = np.array([[0, 1, 2]], dtype=np.int32)
    c = np.array([[255, 0, 0, 255], [0, 255, 0, 255], [0, 0, 255, 255]], dtype=np.uint8)
    out = sr.render(v, f, c, None, CAM, SIZE)
    vd = v.astype(np.float64)
    uv = np.stack([vd[:, 0] / vd[:, 2] * fx + cx, vd[:, 1] / vd[:, 2] * fy + cy], -1)
    n = np.cross(vd[1] - vd[0], vd[2] - vd[0])
    n /= np.linalg.norm(n)
    shade = sr.AMBIENT + sr.DIFFUSE * abs(n[2])
    checked = 0
    for b in ((1 / 3, 1 / 3, 1 / 3), (0.6, 0.3, 0.1), (0.1, 0.2, 0.7)):
        x, y = (int(math.floor(k)) for k in np.asarray(b) @ uv)
        s = np.array([x + 0.5, y + 0.5])
        m = np.array([[uv[0, 0], uv[1, 0], uv[2, 0]], [uv[0, 1], uv[1, 1], uv[2, 1]], [1, 1, 1]])
        beta = np.linalg.solve(m, [s[0], s[1], 1.0])
        assert (beta > 0.02).all()
        lam = beta / vd[:, 2] / (beta / vd[:, 2]).sum()
        assert out['face_id'][y, x] == 0
        assert np.allclose(out['weights'][y, x], lam, atol=1e-12)
        assert abs(out['depth'][y, x] - 1.0 / (beta / vd[:, 2]).sum()) < 1e-12
        exact = 255.0 * lam * shade
        want = np.floor(np.minimum(255.0, exact) + 0.5)
        near_half = np.abs(exact - np.floor(exact) - 0.5) < 1e-9
        assert (np.abs(out['rgba'][y, x, :3].astype(int) - want) <= near_half).all()
        assert out['rgba'][y, x, 3] == 255
        assert not np.allclose(lam, beta, atol=0.02)          # the affine weights would be wrong
        checked += 1
    assert checked == 3


def test_coincident_faces_the_lower_index_wins():
    v, f = rr.quad((-0.5, -0.4, 3.0), (0.5, -0.4, 3.0), (0.5, 0.4, 3.0), (-0.5, 0.4, 3.0))
    v2, f2 = np.concatenate([v, v]), np.concatenate([f, f + 4])
    red, blue = np.tile(np.uint8([255, 0, 0, 255]), (4, 1)), np.tile(np.uint8([0, 0, 255, 255]), (4, 1))
    out = sr.render(v2, f2, np.concatenate([red, blue]), None, CAM, SIZE)
    hit = out['face_id'] >= 0
    assert hit.sum() > 5000 and (out['face_id'][hit] <= 1).all()
    assert (out['rgba'][hit][:, 0] == 255).all() and (out['rgba'][hit][:, 2] == 0).all()
    assert (out['gap'][hit] == 0).all()
    out = sr.render(v2, np.concatenate([f + 4, f]), np.concatenate([red, blue]), None, CAM, SIZE)
    assert (out['rgba'][hit][:, 2] == 255).all() and (out['rgba'][hit][:, 0] == 0).all()


# ---- image arithmetic and PNG -----------------------------------------------------------------------------------------
def _all_pairs():
    val, a = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing='ij')
    return val, a


@pytest.mark.parametrize('mode', ['RGB', 'RGBA'])
def test_paste_matches_pil(mode):
    Image = pytest.importorskip('PIL.Image')
    val, a = _all_pairs()
    g = np.random.Generator(np.random.PCG64(3))
    src = np.stack([val, g.integers(0, 256, val.shape, dtype=np.uint8), 255 - val, a], -1)
    dst = g.integers(0, 256, (256, 256, len(mode)), dtype=np.uint8)
    im = Image.fromarray(dst, mode)
    s = Image.fromarray(src, 'RGBA')
    im.paste(s, (0, 0), s)
    assert np.array_equal(np.asarray(im), sr.paste(dst, src))


@pytest.mark.parametrize('alpha', [1.0, 0.9, 0.5])
def test_requantize_is_render_img(alpha):
    color = np.tile(np.arange(256, dtype=np.uint8)[:, None, None], (1, 3, 4))
    want = color.astype(np.float32) / 255.0
    want[:, :, -1] = want[:, :, -1] * alpha
    want = (want * 255).astype(np.uint8)
    assert np.array_equal(sr.requantize(color, alpha), want)
    assert (want[..., :3] <= color[..., :3]).all()          # the round trip may lose a level, never gain one


def test_overlay_and_flip():
    g = np.random.Generator(np.random.PCG64(4))
    dst = g.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    src = g.integers(0, 256, (5, 7, 4), dtype=np.uint8)
    src[::2, ::3, 3] = 0
    valid = (src[:, :, -1] > 0)[:, :, np.newaxis]
    assert np.array_equal(sr.overlay(dst, src), (src[:, :, :-1] * valid + (1 - valid) * dst).astype(np.uint8))
    assert np.array_equal(sr.flip_lr(src)[:, 0], src[:, -1]) and np.array_equal(sr.flip_lr(sr.flip_lr(src)), src)


def _decode_png(blob):
    """Standard-library decoder for what write_png writes: 8-bit RGB / RGBA, no interlace, filter 0 on every row."""
    assert blob[:8] == b'\x89PNG\r\n\x1a\n'
    at, chunks = 8, []
    while at < len(blob):
        n, tag = struct.unpack('>I4s', blob[at:at + 8])
        data = blob[at + 8:at + 8 + n]
        assert struct.unpack('>I', blob[at + 8 + n:at + 12 + n])[0] == zlib.crc32(tag + data) & 0xffffffff
        chunks.append((tag, data))
        at += 12 + n
    assert chunks[0][0] == b'IHDR' and chunks[-1][0] == b'IEND'
    Wd, Ht, depth, ctype, comp, flt, lace = struct.unpack('>IIBBBBB', chunks[0][1])
    assert (depth, comp, flt, lace) == (8, 0, 0, 0) and ctype in (2, 6)
    C = 4 if ctype == 6 else 3
    raw = zlib.decompress(b''.join(d for t, d in chunks if t == b'IDAT'))
    rows = np.frombuffer(raw, np.uint8).reshape(Ht, 1 + Wd * C)
    out = np.zeros((Ht, Wd * C), np.uint8)
    for y in range(Ht):
        assert rows[y, 0] == 0          # write_png uses filter 0 throughout
        out[y] = rows[y, 1:]
    return out.reshape(Ht, Wd, C)


@pytest.mark.parametrize('channels', [3, 4])
def test_write_png_round_trips(tmp_path, channels):
    g = np.random.Generator(np.random.PCG64(5))
    img = g.integers(0, 256, (37, 53, channels), dtype=np.uint8)
    path = tmp_path / 'a.png'
    R.write_png(str(path), img)
    assert np.array_equal(_decode_png(path.read_bytes()), img)
    try:
        from PIL import Image
    except ImportError:
        return
    with Image.open(path) as im:
        assert im.mode == ('RGBA' if channels == 4 else 'RGB')
        assert np.array_equal(np.asarray(im), img)


# ---- host builders ------------------------------------------------------------------------------------------------------
def test_floor_mesh_is_the_checkerboard():
    v, f, c = R.floor_mesh()
    assert v.shape == (10000, 3) and f.shape == (5000, 3) and c.shape == (10000, 4)
    assert (v[:, 2] == 0).all() and v[:, :2].min() == -12.5 and v[:, :2].max() == 12.5
    assert len(np.unique(f)) == 10000                                         # no vertex shared between tiles
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert np.allclose(n, [0, 0, 0.25])                                        # two 0.125 m^2 halves per tile, facing up
    tiles = c.reshape(50, 50, 4, 4)
    assert (tiles == tiles[:, :, :1]).all()
    i, j = np.meshgrid(np.arange(50), np.arange(50), indexing='ij')
    even = (i % 2) == (j % 2)
    assert (tiles[even][:, 0] == np.uint8([204, 230, 230, 255])).all()
    assert (tiles[~even][:, 0] == np.uint8([153, 178, 178, 255])).all()
    # tile (i, j) starts at (-12.5 + 0.5 j, 12.5 - 0.5 i), as create_floor lays them out
    assert np.allclose(v.reshape(50, 50, 4, 3)[3, 7, 0], [-12.5 + 3.5, 12.5 - 1.5, 0])
    trans = np.array([[0, 0, -1, 5], [-1, 0, 0, 1], [0, -1, 0, 1], [0, 0, 0, 1]], dtype=np.float64)
    moved = R.floor_mesh(trans)[0]
    back = moved.astype(np.float64) @ trans[:3, :3].T + trans[:3, 3]
    assert np.allclose(back, v, atol=1e-5)


@pytest.mark.parametrize('sub', [0, 1, 3])
def test_icosphere(sub):
    v, f = R.icosphere(sub)
    assert len(v) == 10 * 4 ** sub + 2 and len(f) == 20 * 4 ** sub
    assert np.allclose(np.linalg.norm(v, axis=1), 1.0, atol=1e-6)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert ((n * v[f].mean(1)).sum(1) > 0).all()
    edges = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    assert (np.unique(edges, axis=0, return_counts=True)[1] == 2).all()          # closed


@pytest.mark.parametrize('sections', [3, 8, 32])
def test_cylinder(sections):
    v, f = R.cylinder(sections)
    assert len(v) == 2 + 2 * sections and len(f) == 4 * sections
    assert v[:, 2].min() == 0 and v[:, 2].max() == 1
    assert np.allclose(np.linalg.norm(v[2:, :2], axis=1), 1.0, atol=1e-6)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert ((n * (v[f].mean(1) - [0, 0, 0.5])).sum(1) > 0).all()
    edges = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    assert (np.unique(edges, axis=0, return_counts=True)[1] == 2).all()


def test_merge_and_adjacency():
    a = (np.zeros((3, 3), np.float32), np.array([[0, 1, 2]]), np.full((3, 4), 7, np.uint8))
    b = (np.ones((4, 3), np.float32), np.array([[0, 1, 2], [0, 2, 3]]), np.full((4, 4), 9, np.uint8))
    v, f, c = R.merge(a, b)
    assert v.shape == (7, 3) and f.tolist() == [[0, 1, 2], [3, 4, 5], [3, 5, 6]] and c[:, 0].tolist() == [7] * 3 + [9] * 4
    off, ids = R.vertex_adjacency(f, 8)
    assert off.tolist() == [0, 1, 2, 3, 5, 6, 8, 9, 9] and ids.tolist() == [0, 0, 0, 1, 2, 1, 1, 2, 2]


M = {k: list(v) for k, v in R.MATERIALS.items()}
LIMBS = np.asarray(R.LIMBS_BODY_SMPL)


def test_material_table_and_limbs():
    assert M['body_rec_vis'] == [66, 149, 245, 255] and M['contact_1'] == [0, 139, 0, 255] and M['joint_occ'] == [222, 177, 4, 255]
    assert len(LIMBS) == 21 and sorted(set(LIMBS.ravel().tolist())) == list(range(22)) and R.LIMBS_BODY_SMPL == sr.LIMBS
    assert LIMBS[0].tolist() == [15, 12] and LIMBS[-1].tolist() == [8, 11]


@pytest.mark.parametrize('scheme', ['lower', 'video'])
@pytest.mark.parametrize('add_occ', [True, False])
@pytest.mark.parametrize('contact', [True, False])
def test_skeleton_colors_joint_schemes(scheme, add_occ, contact):
    T = 3
    mask = [1, 2, 4, 5, 7, 8, 10, 11]
    lbl = np.array([[1, 0, 1, 0], [0, 0, 0, 0], [1, 1, 1, 1]])
    arg = mask
    if scheme == 'video':          # per frame: frame 1 has nothing occluded
        arg = np.zeros((T, 22), bool)
        arg[0, mask] = arg[2, mask] = True
    col, hide = R.skeleton_colors(T, scheme, arg, add_occ, add_contact=contact, contact_lbl=lbl if contact else None)
    assert col.shape == (T, 43, 4) and hide.shape == (T, 43) and col.dtype == np.uint8
    for t in range(T):
        occ = set(mask) if (scheme == 'lower' or t != 1) else set()
        for j in range(22):
            if contact and j in (7, 10, 8, 11):
                want = M['contact_1'] if lbl[t, {7: 0, 10: 1, 8: 2, 11: 3}[j]] == 1 else M['contact_0']
            else:
                want = M['joint_occ'] if j in occ else M['joint_vis']
            assert col[t, j].tolist() == want
            assert hide[t, j] == (not add_occ and j in occ)
        for l, (a, b) in enumerate(LIMBS):
            touched = a in occ or b in occ
            assert col[t, 22 + l].tolist() == (M['joint_occ'] if touched else M['skel_vis'])
            assert hide[t, 22 + l] == (not add_occ and touched)


@pytest.mark.parametrize('add_occ', [True, False])
@pytest.mark.parametrize('contact', [True, False])
def test_skeleton_colors_full_scheme(add_occ, contact):
    T, start, end = 6, 2, 4
    lbl = np.tile([1, 0, 0, 1], (T, 1))
    col, hide = R.skeleton_colors(T, 'full', None, add_occ, start, end, contact, lbl if contact else None)
    assert not hide.any()                                   # 'full' never omits a primitive
    for t in range(T):
        inside = start <= t < end
        for j in range(22):
            if contact and j in (7, 10, 8, 11):
                want = M['contact_1'] if j in (7, 11) else M['contact_0']
            else:
                want = M['joint_occ'] if inside else M['joint_vis']
            assert col[t, j].tolist() == want
        assert (col[t, 22:] == np.uint8(M['joint_occ'] if inside else M['skel_vis'])).all()
    with pytest.raises(ValueError):
        R.skeleton_colors(1, 'upper')


def test_restated_normals_and_skeleton():
    v, f = R.icosphere(0)                                   # an icosahedron: by symmetry every vertex normal is radial
    n = sr.vertex_normals(np.concatenate([v, [[9, 9, 9]]]), f)
    assert np.allclose(n[:-1], v, atol=1e-6) and (n[-1] == 0).all()
    sv, _ = R.icosphere(1)
    cv, _ = R.cylinder(6)
    j = np.zeros((1, 22, 3))
    j[0, :, 0] = np.arange(22) * 0.1
    j[0, 12] = j[0, 15]                                     # limb 0 has zero length
    hide = np.zeros((1, 43), np.uint8)
    hide[0, 3] = hide[0, 22 + 5] = 1
    out = sr.skeleton_mesh(j, sv, cv, hide=hide)
    Vs, Vc = len(sv), len(cv)
    assert out.shape == (1, 22 * Vs + 21 * Vc, 3)
    assert np.allclose(np.linalg.norm(out[0, :Vs] - j[0, 0], axis=1), 0.025)
    assert (out[0, 3 * Vs:4 * Vs] == j[0, 3]).all()
    assert (out[0, 22 * Vs:22 * Vs + Vc] == j[0, 15]).all()
    c5 = out[0, 22 * Vs + 5 * Vc:22 * Vs + 6 * Vc]
    assert (c5 == j[0, LIMBS[5][0]]).all()
    c12 = out[0, 22 * Vs + 12 * Vc:22 * Vs + 13 * Vc]       # (3, 0): along -x, length 0.3
    p1, p2 = j[0, 3], j[0, 0]
    axis = (p2 - p1) / np.linalg.norm(p2 - p1)
    along = (c12 - p1) @ axis
    assert np.allclose(along[[0, 1]], [0, 0.3]) and along.min() > -1e-12 and along.max() < 0.3 + 1e-12
    radial = np.linalg.norm((c12 - p1) - along[:, None] * axis, axis=1)
    assert np.allclose(radial[2:], 0.01)
