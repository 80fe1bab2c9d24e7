"""GPU: the colour renderer, vertex normals, skeleton mesh and image arithmetic of csrc/shade.hip / rohm_amd.render, and the
`--render` path of `python -m rohm_amd.evaluation`, against the float64 restatement tests/shade_ref.py (itself checked
against closed forms in tests/test_shade_ref.py).  pyrender exists neither where this project is built nor on the GPU
machines: nothing is pinned to it.

Bars.  Pictures are 480 x 270 under raster_ref.PROX_CAM / 4.  A pixel is compared if its sample lies at least
EDGE_BAND = 1e-3 px from every edge (the depth tests' band) and if, in the restatement, the two nearest hits along its ray
differ by at least TIE_BAND = 1e-4 m (closer than that, float32 depths may order the other way); the edge band may take
at most 1 % of the covered pixels, the tie band at most 0.5 %.  On compared pixels face_id is equal, depth is within
1e-4 m, and every rgba channel is within 1 level: fp32 shading error is about 1e-6 of a 1 / 255 step, so the two differ
only where a value sits on a rounding boundary.  The measured figures go to profiles/render_parity.json.
"""
import json
import os
import pickle
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

import raster_ref as rr
import shade_ref as sr
from raster_scenes import sphere_body, walking_params, write_npz

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = tuple(v / 4 for v in rr.PROX_CAM)
SIZE = (480, 270)
W, H = SIZE
EDGE_BAND, TIE_BAND, DEPTH_BAR = 1e-3, 1e-4, 1e-4
QUARTER = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], dtype=np.float64)
PARITY = {}


def _R():
    from rohm_amd import render
    return render


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _record(key, value):
    PARITY[key] = value
    try:
        with open(os.path.join(ROOT, 'profiles', 'render_parity.json'), 'w') as f:
            json.dump(PARITY, f, indent=1, sort_keys=True)
            f.write('\n')
    except OSError:
        pass


def _compare(gpu_rgba, gpu_depth, gpu_face, ref, edge):
    covered = ref['face_id'] >= 0
    clear = edge >= EDGE_BAND
    tie = covered & clear & (ref['gap'] < TIE_BAND)
    cmp_ = clear & ~tie
    both = cmp_ & covered & (gpu_face >= 0)
    diff = np.abs(gpu_rgba.astype(np.int64) - ref['rgba'].astype(np.int64)).max(-1)
    return {
        'covered': int(covered.sum()),
        'edge_excluded_share': float((covered & ~clear).sum() / max(1, covered.sum())),
        'tie_excluded_share': float(tie.sum() / max(1, covered.sum())),
        'hit_miss_mismatches': int((cmp_ & ((gpu_face >= 0) != covered)).sum()),
        'face_id_mismatches': int((cmp_ & (gpu_face != ref['face_id'])).sum()),
        'max_abs_depth_err': float(np.abs(gpu_depth.astype(np.float64) - ref['depth'])[both].max()) if both.any() else 0.0,
        'max_level_diff': int(diff[cmp_].max()),
        'differing_share': float((diff[cmp_] > 0).sum() / max(1, cmp_.sum())),
    }


def _check(fig, min_covered):
    assert fig['covered'] > min_covered
    assert fig['edge_excluded_share'] <= 0.01
    assert fig['tie_excluded_share'] <= 0.005
    assert fig['hit_miss_mismatches'] == 0
    assert fig['face_id_mismatches'] == 0
    assert fig['max_abs_depth_err'] <= DEPTH_BAR
    assert fig['max_level_diff'] <= 1


def scene_mesh():
    return rr.merge(rr.uv_sphere(16, 32, 0.5, (0.1, -0.05, 3.0)), rr.uv_sphere(12, 24, 0.4, (0.55, 0.1, 2.9)),
                    rr.height_field(40, 3.2, amp=0.3))


@pytest.fixture(scope='module')
def scene():
    """Two meshes (the second the first moved by an exact quarter turn, with its own colours), device normals and renders."""
    R = _R()
    v, f = scene_mesh()
    assert len(f) == 4642
    v2 = (v.astype(np.float64) @ QUARTER.T).astype(np.float32)
    verts = np.stack([v, v2])
    g = np.random.Generator(np.random.PCG64(7))
    colors = g.integers(0, 256, (2, len(v), 4), dtype=np.uint8)
    normals = R.vertex_normals(_dev(verts), f)
    rgba, depth, face = R.color_render(_dev(verts), f, _dev(colors), CAM, SIZE, normals=normals, with_depth=True, with_face_id=True)
    return dict(verts=verts, faces=f, colors=colors, normals=normals, rgba=rgba, depth=depth, face=face)


def test_scene_matches_restatement(scene):
    normals = scene['normals'].cpu().numpy()
    winners = set()
    for i in range(2):
        v = scene['verts'][i]
        ref = sr.render(v, scene['faces'], scene['colors'][i], normals[i], CAM, SIZE)
        edge = rr.edge_distance(v, scene['faces'], CAM, SIZE)
        fig = _compare(scene['rgba'][i].cpu().numpy(), scene['depth'][i].cpu().numpy(), scene['face'][i].cpu().numpy(), ref, edge)
        print(i, fig)
        _record(f'scene_mesh{i}', fig)
        _check(fig, 20000)
        ids = ref['face_id'][ref['face_id'] >= 0]
        winners |= {int(k) for k in np.unique(np.digitize(ids, [1024, 1600]))}
    assert winners == {0, 1, 2}                               # each of the three interpenetrating surfaces wins somewhere
    assert not torch.equal(scene['rgba'][0], scene['rgba'][1])


def _box():
    v, f = rr.box()
    verts = v[f].reshape(-1, 3)                               # unshared vertices: one colour per face
    faces = np.arange(36, dtype=np.int32).reshape(12, 3)
    g = np.random.Generator(np.random.PCG64(8))
    colors = np.repeat(g.integers(0, 256, (12, 4), dtype=np.uint8), 3, axis=0)
    return verts, faces, colors


def test_box_around_the_camera_flat_shaded():
    R = _R()
    v, f, c = _box()
    rgba, depth, face = R.color_render(_dev(v), f, _dev(c), CAM, SIZE, normals=None, with_depth=True, with_face_id=True)
    ref = sr.render(v, f, c, None, CAM, SIZE)
    edge = rr.edge_distance(v, f, CAM, SIZE)
    fig = _compare(rgba[0].cpu().numpy(), depth[0].cpu().numpy(), face[0].cpu().numpy(), ref, edge)
    print(fig)
    _record('box', fig)
    _check(fig, 100000)
    assert len(np.unique(ref['face_id'])) >= 4


def test_depth_output_is_depth_render_bit_for_bit(scene):
    from rohm_amd import occlusion
    R = _R()
    d = occlusion.depth_render(_dev(scene['verts']), scene['faces'], CAM, SIZE)
    assert torch.equal(d.view(torch.int32), scene['depth'].view(torch.int32))
    assert torch.equal(scene['face'] >= 0, d > 0)
    v, f, c = _box()
    got = R.color_render(_dev(v), f, _dev(c), CAM, SIZE, with_depth=True)[1]
    assert torch.equal(got.view(torch.int32), occlusion.depth_render(_dev(v), f, CAM, SIZE).view(torch.int32))
    v, f = rr.uv_sphere(64, 128)
    c = _dev(np.full((len(v), 4), 200, np.uint8))
    rgba, got, _ = R.color_render(_dev(v), f, c, rr.PROX_CAM, rr.PROX_SIZE, with_depth=True)
    want = occlusion.depth_render(_dev(v), f, rr.PROX_CAM, rr.PROX_SIZE)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and int((want > 0).sum()) > 100000
    assert torch.equal(rgba[..., 3] > 0, want > 0)
    # culled: the covered set is depth_render's culled one
    v, f = scene['verts'], scene['faces']
    _, dc, fc = R.color_render(_dev(v), f, _dev(scene['colors']), CAM, SIZE, cull_backfaces=True, with_depth=True, with_face_id=True)
    want = occlusion.depth_render(_dev(v), f, CAM, SIZE, cull_backfaces=True)
    assert torch.equal(dc.view(torch.int32), want.view(torch.int32)) and torch.equal(fc >= 0, want > 0)
    assert not torch.equal(want, d)


def test_render_is_bitwise_reproducible(scene):
    R = _R()
    rgba, depth, face = R.color_render(_dev(scene['verts']), scene['faces'], _dev(scene['colors']), CAM, SIZE,
                                       normals=scene['normals'], with_depth=True, with_face_id=True)
    assert torch.equal(rgba, scene['rgba']) and torch.equal(face, scene['face'])
    assert torch.equal(depth.view(torch.int32), scene['depth'].view(torch.int32))


def test_tie_rule_the_lowest_face_index_wins():
    R = _R()
    v, f = rr.quad((-0.5, -0.4, 3.0), (0.5, -0.4, 3.0), (0.5, 0.4, 3.0), (-0.5, 0.4, 3.0))
    v2 = np.concatenate([v, v])
    red, blue = np.tile(np.uint8([255, 0, 0, 255]), (4, 1)), np.tile(np.uint8([0, 0, 255, 255]), (4, 1))
    c = _dev(np.concatenate([red, blue]))
    for faces, (lo, hi) in ((np.concatenate([f, f + 4]), (0, 2)), (np.concatenate([f + 4, f]), (2, 0))):
        rgba, _, face = R.color_render(_dev(v2), faces, c, CAM, SIZE, with_face_id=True)
        hit = face[0] >= 0
        assert int(hit.sum()) > 5000
        px = rgba[0][hit]
        assert bool((px[:, lo] == 255).all()) and bool((px[:, hi] == 0).all())
        assert int(face[0][hit].max()) <= 1


def test_vertex_normals(scene):
    R = _R()
    v, f = scene_mesh()
    v = np.concatenate([v, [[9.0, 9.0, 9.0]]]).astype(np.float32)          # referenced by no face
    a, b = R.vertex_normals(_dev(v), f), R.vertex_normals(_dev(v), f)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    got = a[0].cpu().numpy()
    want = sr.vertex_normals(v, f)
    err = float(np.abs(got - want).max())
    print('normals max err', err)
    _record('normals_max_abs_err', err)
    assert err <= 1e-5
    assert (got[-1] == 0).all() and np.allclose(np.linalg.norm(got[:-1], axis=1), 1.0, atol=1e-5)
    assert torch.equal(scene['normals'][0], a[0, :-1])


# ---- skeleton -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def body(tmp_path_factory):
    from rohm_amd.body_model import SMPLXLayer
    root = tmp_path_factory.mktemp('render')
    tensors, faces = sphere_body()
    npz = str(root / 'SMPLX_NEUTRAL.npz')
    write_npz(npz, tensors, faces)
    return dict(root=root, npz=npz, tensors=tensors, faces=faces, layer=SMPLXLayer.from_npz(npz).to(DEV))


def test_skeleton_mesh(body):
    from rohm_amd.body_model import lbs_forward, native_for
    R = _R()
    n = 8
    params = walking_params(body['tensors'], n=n)
    nat = native_for(body['layer'], torch.device(DEV))
    pose = torch.cat([_dev(params['global_orient']).reshape(n, 1, 3), _dev(params['body_pose']).reshape(n, 21, 3)], 1)
    joints = lbs_forward(nat, pose.contiguous(), 0, _dev(params['betas']), _dev(params['transl']))[0][:, :22].contiguous()
    joints[:, 20] = joints[:, 18]                              # limb (18, 20) has zero length
    sv, sf = R.icosphere(1)
    cv, cf = R.cylinder(8)
    Vs, Vc, Fs, Fc = len(sv), len(cv), len(sf), len(cf)
    hide = np.zeros((n, 43), np.uint8)
    hidden = [3, 16, 22 + 13]                                  # two joints and limb (0, 1)
    hide[:, hidden] = 1
    verts = R.skeleton_mesh(joints, sv, cv, hide=hide)
    j_host = joints.cpu().numpy()
    want = sr.skeleton_mesh(j_host, sv, cv, hide=hide)
    got = verts.cpu().numpy()
    err = float(np.abs(got - want).max())
    print('skeleton max err', err)
    _record('skeleton_max_abs_err_m', err)
    assert got.shape == (n, 22 * Vs + 21 * Vc, 3) and err <= 1e-6
    sl = lambda p: slice(p * Vs, (p + 1) * Vs) if p < 22 else slice(22 * Vs + (p - 22) * Vc, 22 * Vs + (p - 21) * Vc)
    first = {3: 3, 16: 16, 22 + 13: R.LIMBS_BODY_SMPL[13][0], 22 + 4: 18}
    for p, j in first.items():
        assert (got[:, sl(p)] == j_host[:, j][:, None]).all()
    # one face list for the batch; the collapsed primitives draw nothing
    tmpl = R.SkeletonTemplate(torch.device(DEV), 1, 8)
    assert tmpl.n_verts == got.shape[1] and len(tmpl.faces) == 22 * Fs + 21 * Fc
    colors = np.full((n, 43, 4), 255, np.uint8)
    vcol = _dev(colors)[:, tmpl.prim].contiguous()
    rgba, _, face = R.color_render(verts, tmpl.faces_d, vcol, CAM, SIZE, normals=R.vertex_normals(verts, tmpl.faces_d, tmpl.adjacency),
                                   with_face_id=True)
    face = face.cpu().numpy()
    prim = np.where(face < 22 * Fs, face // Fs, 22 + (face - 22 * Fs) // Fc)
    prim[face < 0] = -1
    seen = set(np.unique(prim).tolist())
    assert not seen & set(first) and len(seen) > 30 and int((face >= 0).sum()) > 2000


# ---- image arithmetic -------------------------------------------------------------------------------------------------
def _pairs_image():
    val, a = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing='ij')
    g = np.random.Generator(np.random.PCG64(3))
    return np.stack([val, g.integers(0, 256, val.shape, dtype=np.uint8), 255 - val, a], -1), g


@pytest.mark.parametrize('channels', [3, 4])
def test_paste_bit_for_bit(channels):
    src, g = _pairs_image()
    # every (source value, alpha) pair, four random destinations each
    dst = g.integers(0, 256, (4, 256, 256, channels), dtype=np.uint8)
    srcs = np.tile(src[None], (4, 1, 1, 1))
    got = _R().paste(_dev(dst), _dev(srcs)).cpu().numpy()
    assert np.array_equal(got, sr.paste(dst, srcs))
    assert got.shape == dst.shape


def test_overlay_and_flip_bit_for_bit():
    src, g = _pairs_image()
    dst = g.integers(0, 256, (256, 256, 3), dtype=np.uint8)
    R = _R()
    assert np.array_equal(R.overlay(_dev(dst), _dev(src)).cpu().numpy(), sr.overlay(dst, src))
    odd = g.integers(0, 256, (3, 5, 7, 4), dtype=np.uint8)
    assert np.array_equal(R.flip_lr(_dev(odd)).cpu().numpy(), sr.flip_lr(odd))
    assert np.array_equal(R.flip_lr(_dev(dst)).cpu().numpy(), sr.flip_lr(dst))


@pytest.mark.parametrize('alpha', [1.0, 0.9, 0.5])
def test_requantize_bit_for_bit(alpha):
    src, _ = _pairs_image()
    assert np.array_equal(_R().requantize(_dev(src), alpha).cpu().numpy(), sr.requantize(src, alpha))


# ---- end to end -------------------------------------------------------------------------------------------------------
def _decode_png(path):
    blob = open(path, 'rb').read()
    at, idat, head = 8, b'', None
    while at < len(blob):
        n, tag = struct.unpack('>I4s', blob[at:at + 8])
        if tag == b'IHDR':
            head = struct.unpack('>IIBBBBB', blob[at + 8:at + 8 + n])
        elif tag == b'IDAT':
            idat += blob[at + 8:at + 8 + n]
        at += 12 + n
    Wd, Ht, _, ctype = head[:4]
    C = 4 if ctype == 6 else 3
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(Ht, 1 + Wd * C)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(Ht, Wd, C)


def test_evaluator_renders_amass_end_to_end(body, tmp_path, capsys):
    from rohm_amd import evaluation as E
    from rohm_amd.data_loaders.motion_representation import REPR_DIM_DICT, REPR_LIST, joints_from_repr
    from rohm_amd.utils import synth
    R = _R()
    n_seq, T = 2, 4
    mean, std = synth.synthetic_stats(0)
    # the walk's facing direction comes from the plain synthetic body (the sphere body's hips and shoulders need not differ)
    x = synth.walking_motion(5, n_seq, T, mean, std, synth.synthetic_smplx_tensors(0, num_verts=2000)).numpy() * std + mean
    assert np.isfinite(x).all()
    g = np.random.Generator(np.random.PCG64(9))
    clean = x.astype(np.float32)
    rec = (x + 0.01 * g.standard_normal(x.shape) * std).astype(np.float32)
    noisy = (x + 0.03 * g.standard_normal(x.shape) * std).astype(np.float32)
    jt = lambda a: joints_from_repr(_dev(a), 'smplx_params', body['layer']).cpu().numpy()
    data = {'repr_name_list': list(REPR_LIST), 'repr_dim_dict': dict(REPR_DIM_DICT), 'rec_ric_data_clean_list': jt(clean),
            'rec_ric_data_noisy_list': jt(noisy), 'rec_ric_data_rec_list_from_abs_traj': jt(rec),
            'rec_ric_data_rec_list_from_smpl': jt(rec), 'motion_repr_clean_list': clean, 'motion_repr_noisy_list': noisy,
            'motion_repr_rec_list': rec}
    pkl = tmp_path / 'amass.pkl'
    with open(pkl, 'wb') as f:
        pickle.dump(data, f)
    out = tmp_path / 'pictures'
    common = ['--dataset', 'amass', '--saved_data_path', str(pkl), '--mask_scheme', 'lower']
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'rohm_amd.evaluation', *common, '--render', 'True', '--render_interval', '1',
                        '--render_save_path', str(out), '--body_model_path', body['npz'], '--render_size', '480', '270'],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert E.main(common) == 0
    assert r.stdout == capsys.readouterr().out                 # the metric lines do not change with --render
    want = R.render_amass(data, body['layer'], 'lower', 0.0, None, 1, SIZE, device=DEV, return_images=True)
    for kind in ('pred', 'input', 'gt'):
        for bs in range(n_seq):
            for t in range(T):
                path = out / kind / f'seq_{bs:03d}' / f'frame_{t:03d}.png'
                assert path.is_file(), path
                assert np.array_equal(_decode_png(path), want[kind][bs][t]), path
    assert sum(len(files) for _, _, files in os.walk(out)) == n_seq * T * 3
    # pred and gt: the same picture but for the body's material (and the skeleton pasted over pred).  Off the body and the
    # skeleton they are equal; on the body the green channel of gt, 102 / 255 x shade, never saturates and gives the shade
    # back: 102 shade lies in [g - 0.5, g + 1.5] (rounding, and render_img's round trip may have lost a level), and pred's
    # channel k, C_k shade rounded and possibly one level lower, lies in [C_k shade - 1.5, C_k shade + 0.5].
    C = np.asarray(R.MATERIALS['body_rec_vis'][:3], dtype=np.float64)
    bodies = 0
    for bs in range(n_seq):
        pred, gt = want['pred'][bs].astype(np.float64), want['gt'][bs].astype(np.float64)
        on_body, on_skel = want['body_mask'][bs], want['skeleton_mask'][bs]
        assert (pred[~on_body & ~on_skel] == gt[~on_body & ~on_skel]).all()
        m = on_body & ~on_skel
        bodies += int(m.sum())
        lo = np.minimum(255.0, C[None] * (gt[m][:, 1:2] - 0.5) / 102.0) - 1.5
        hi = np.minimum(255.0, C[None] * (gt[m][:, 1:2] + 1.5) / 102.0) + 0.5
        assert ((pred[m][:, :3] >= lo - 1e-9) & (pred[m][:, :3] <= hi + 1e-9)).all()
        assert (pred[m][:, 3] == 255).all() and (gt[m][:, 3] == 255).all()
        assert int(on_skel.sum()) > 50
        assert not np.array_equal(want['input'][bs], want['pred'][bs])
    assert bodies > 2000


def test_scene_clips_and_the_prox_evaluator(body, tmp_path, capsys):
    """render_scene_clips (eval_prox_egobody.py:415-443) on a synthetic recording: off the bodies and the skeleton the
    pictures are the background, the body is pasted at alpha 0.9 (render_img, then Image.paste) and the input body overlaid
    opaquely; then `--dataset prox --render` in process writes exactly these pictures under mesh_skel/ and input/."""
    from rohm_amd import evaluation as E
    from rohm_amd.data_loaders.motion_representation import REPR_DIM_DICT, REPR_LIST, joints_from_repr
    from rohm_amd.utils import synth
    R = _R()
    n_seq, T = 2, 3
    mean, std = synth.synthetic_stats(0)
    x = synth.walking_motion(6, n_seq, T, mean, std, synth.synthetic_smplx_tensors(0, num_verts=2000)).numpy() * std + mean
    g = np.random.Generator(np.random.PCG64(10))
    rec, noisy = x.astype(np.float32), (x + 0.05 * g.standard_normal(x.shape) * std).astype(np.float32)
    joints = joints_from_repr(_dev(rec), 'smplx_params', body['layer']).cpu().numpy()
    mask = (g.random((n_seq, T, 22)) > 0.3).astype(np.float32)
    # canonical -> scene is a quarter turn about z and a shift; the camera looks along scene -x from 4 m, as AMASS's does
    s2c = np.tile(np.array([[0, 1, 0, 0.5], [-1, 0, 0, 0.25], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float32), (n_seq, 1, 1))
    cam2world = np.linalg.inv(s2c[0].astype(np.float64)) @ np.array([[0, 0, -1, 4.0], [-1, 0, 0, 0.5], [0, -1, 0, 1.0], [0, 0, 0, 1]])
    data = {'repr_name_list': list(REPR_LIST), 'repr_dim_dict': dict(REPR_DIM_DICT), 'rec_ric_data_rec_list_from_smpl': joints,
            'rec_ric_data_noisy_list': joints, 'motion_repr_rec_list': rec, 'motion_repr_noisy_list': noisy,
            'mask_joint_vis_list': mask, 'trans_scene2cano_list': s2c}
    f, c = (265.0, 265.0), (240.0, 135.0)
    bg = g.integers(0, 256, (n_seq, T, H, W, 3), dtype=np.uint8)
    v_rec = torch.stack([R._clip_verts(data, 'motion_repr_rec_list', i, body['layer'], DEV) for i in range(n_seq)])
    v_in = torch.stack([R._clip_verts(data, 'motion_repr_noisy_list', i, body['layer'], DEV) for i in range(n_seq)])
    contact = rec[:, :, -4:] > 0.5
    kw = dict(mask_joint_vis=mask, contact_lbl=contact, trans_scene2cano=s2c, size=SIZE, skeleton_detail=(1, 8))
    run = lambda j, background: [t.cpu().numpy() for t in R.render_scene_clips(v_rec, v_in, _dev(j), body['faces'], cam2world, f, c,
                                                                               background=background, **kw)]
    behind = np.tile(np.float32([50.0, 0.0, 0.0]), (n_seq, T, 22, 1))          # every joint behind the camera: no skeleton is drawn
    got_rec, got_in = run(joints, _dev(bg))
    black_rec, black_in = run(joints, None)
    nosk_rec, _ = run(behind, _dev(bg))
    nosk_black, _ = run(behind, None)
    assert got_rec.shape == (n_seq, T, H, W, 3) and got_rec.dtype == np.uint8
    on_body = nosk_black.any(-1)
    assert 1000 < on_body.sum() < on_body.size // 2
    assert (nosk_rec[~on_body] == bg[~on_body]).all()
    # the body at alpha 0.9: render_img leaves int(255 * 0.9) = 229, so Image.paste keeps 26 / 255 of the background
    t = nosk_black[on_body].astype(np.int64) * 255 + bg[on_body].astype(np.int64) * 26
    assert (np.abs(nosk_rec[on_body].astype(np.int64) - (t + 127) // 255) <= 1).all()
    # the skeleton is pasted opaquely on top
    on_skel = (black_rec != nosk_black).any(-1)
    assert on_skel.sum() > 50
    assert (got_rec[~on_skel] == nosk_rec[~on_skel]).all() and (got_rec[on_skel] == black_rec[on_skel]).all()
    # the input body: overlaid where it is, the background elsewhere
    on_in = black_in.any(-1)
    assert on_in.sum() > 1000 and (got_in[~on_in] == bg[~on_in]).all() and (got_in[on_in] == black_in[on_in]).all()

    # the evaluator, in process
    prox = tmp_path / 'PROX'
    for d in ('cam2world', 'calibration'):
        (prox / d).mkdir(parents=True)
    (prox / 'cam2world' / 'TestRoom.json').write_text(json.dumps(cam2world.tolist()))
    (prox / 'calibration' / 'Color.json').write_text(json.dumps({'f': [f[0] * 4, f[1] * 4], 'c': [c[0] * 4, c[1] * 4]}))
    saved = tmp_path / 'results'
    saved.mkdir()
    with open(saved / 'TestRoom_00001_01.pkl', 'wb') as fh:
        pickle.dump(data, fh)
    (tmp_path / 'floor.json').write_text(json.dumps({'TestRoom_00001_01': 0.0}))
    models = tmp_path / 'smplx_model' / 'smplx'
    models.mkdir(parents=True)
    (models / 'SMPLX_NEUTRAL.npz').write_bytes(open(body['npz'], 'rb').read())
    common = ['--dataset', 'prox', '--saved_data_dir', str(saved), '--floor_heights', str(tmp_path / 'floor.json')]
    assert E.main(common) == 0
    plain = capsys.readouterr().out
    out = tmp_path / 'pictures'
    assert E.main(common + ['--render', '--render_interval', '1', '--render_save_path', str(out), '--dataset_root', str(prox),
                            '--body_model_path', str(tmp_path / 'smplx_model'), '--render_size', '480', '270']) == 0
    assert capsys.readouterr().out == plain
    full_rec, full_in = (t.cpu().numpy() for t in R.render_scene_clips(v_rec, v_in, _dev(joints), body['faces'], cam2world, f, c,
                                                                       **dict(kw, skeleton_detail=(3, 32))))
    for k in range(n_seq * T):
        name = 'TestRoom_00001_01_frame_{:05d}.png'.format(k)
        assert np.array_equal(_decode_png(out / 'mesh_skel' / name), full_rec[k // T, k % T])
        assert np.array_equal(_decode_png(out / 'input' / name), full_in[k // T, k % T])
    assert sum(len(files) for _, _, files in os.walk(out)) == 2 * n_seq * T


def test_amass_full_scheme_window(body):
    """'full': inside the [65, 65 + int(ratio * 145)) window the predicted body takes the occluded material and the input
    picture goes through render_img at alpha 0.5 -- int(0.5 * 255) = 127, which Image.paste onto itself leaves at 127."""
    from rohm_amd.data_loaders.motion_representation import REPR_DIM_DICT, REPR_LIST, joints_from_repr
    from rohm_amd.utils import synth
    R = _R()
    T = 68
    mean, std = synth.synthetic_stats(0)
    x = (synth.walking_motion(7, 1, T, mean, std, synth.synthetic_smplx_tensors(0, num_verts=2000)).numpy() * std + mean).astype(np.float32)
    j = joints_from_repr(_dev(x), 'smplx_params', body['layer']).cpu().numpy()
    data = {'repr_name_list': list(REPR_LIST), 'repr_dim_dict': dict(REPR_DIM_DICT), 'rec_ric_data_clean_list': j,
            'rec_ric_data_rec_list_from_smpl': j, 'motion_repr_clean_list': x, 'motion_repr_rec_list': x}
    img = R.render_amass(data, body['layer'], 'full', 2 / 145 + 1e-9, None, 1, (240, 136), device=DEV, return_images=True,
                         skeleton_detail=(1, 8))
    pred, inp, m = img['pred'][0], img['input'][0], img['body_mask'][0] & ~img['skeleton_mask'][0]
    inside = np.zeros(T, bool)
    inside[65:67] = True
    assert m[inside].sum() > 100 and m[~inside].sum() > 1000
    assert (pred[inside][m[inside]][:, 0] > pred[inside][m[inside]][:, 2]).all()          # (212, 189, 102): red over blue
    assert (pred[~inside][m[~inside]][:, 2] > pred[~inside][m[~inside]][:, 0]).all()      # (66, 149, 245): blue over red
    assert set(np.unique(inp[inside][..., 3]).tolist()) == {0, 127}
    assert set(np.unique(inp[~inside][..., 3]).tolist()) == {0, 255}
    assert set(np.unique(pred[..., 3]).tolist()) == {0, 255}
