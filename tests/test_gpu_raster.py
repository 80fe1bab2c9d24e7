"""GPU: the depth renderer, the depth probe and the joint-occlusion mask of csrc/raster.hip / rohm_amd.occlusion
(utils/get_occlusion_mask.py) against the float64 restatement tests/raster_ref.py.

Neither pyrender nor OpenCV exists where this project is built, so no fixture comes from them; the restatement is
checked against closed forms in tests/test_raster_ref.py.

Bars.  Hit / miss and depth are compared at every pixel whose sample lies at least EDGE_BAND = 1e-3 px from every edge
(fp32 edge functions at coordinates near 1920 would carry that much error; the device computes coverage in fp64, the
band is kept as stated); the excluded share may be at most 1 % of the covered samples.  Depth: 1e-4 m absolute, 1/1000 of
the 0.1 m decision threshold and about 200 fp32 ulps at 4 m.  Masks: a (frame, joint) pair is left out if its depth
margin is within 1e-3 m of the threshold, if it falls on an excluded pixel or if its projection is within 1e-3 of an
integer; each band removes about 2 x 1e-3 of a unit-sized range (two coordinates for the last one), edges add the
share above, so at most 2 % of the pairs may be left out.  The measured figures go to profiles/occlusion_parity.json.
"""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import raster_ref as rr
from raster_scenes import N_FRAMES, scene_mesh, sphere_body, walking_params, write_npz

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM, SIZE = rr.PROX_CAM, rr.PROX_SIZE
W, H = SIZE
EDGE_BAND = 1e-3
DEPTH_BAR = 1e-4
K_COLOR = [[1060.53, 0.0, 951.30], [0.0, 1060.38, 536.77], [0.0, 0.0, 1.0]]
DIST = [0.052, -0.044, 0.0009, 0.0016, 0.003]
PARITY = {}


def _occ():
    from rohm_amd import occlusion
    return occlusion


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _record(key, value):
    PARITY[key] = value
    try:
        with open(os.path.join(ROOT, 'profiles', 'occlusion_parity.json'), 'w') as f:
            json.dump(PARITY, f, indent=1, sort_keys=True)
            f.write('\n')
    except OSError:
        pass


def _compare(gpu, ref, edge):
    """-> dict of figures; gpu float32 [H, W], ref / edge float64 [H, W]."""
    gpu = gpu.astype(np.float64)
    covered = ref > 0
    clear = edge >= EDGE_BAND
    both = clear & covered & (gpu > 0)
    return {
        'covered': int(covered.sum()),
        'excluded': int((covered & ~clear).sum()),
        'excluded_share': float((covered & ~clear).sum() / max(1, covered.sum())),
        'hit_miss_mismatches': int((clear & ((gpu > 0) != covered)).sum()),
        'max_abs_depth_err': float(np.abs(gpu - ref)[both].max()) if both.any() else 0.0,
    }


MESHES = {
    'sphere': lambda: rr.uv_sphere(64, 128, 0.5, (0.0, 0.0, 3.0)),
    'field': lambda: rr.height_field(200, 4.0),
    'box': lambda: rr.box(),
}
N_FACES = {'sphere': 16384, 'field': 79202, 'box': 12}


@pytest.mark.parametrize('name', ['sphere', 'field', 'box'])
def test_depth_matches_restatement(name):
    v, f = MESHES[name]()
    assert len(f) == N_FACES[name]
    if name == 'box':
        z = v[f][:, :, 2]
        assert (z.max(1) < 0).any() and ((z.min(1) < 0) & (z.max(1) > rr.ZNEAR)).any()
    gpu = _occ().depth_render(_dev(v), f, CAM, SIZE)[0].cpu().numpy()
    ref, edge = rr.render(v, f, CAM, SIZE, with_edges=True)
    fig = _compare(gpu, ref, edge)
    print(name, fig)
    _record('depth_' + name, fig)
    assert fig['covered'] > 50000
    assert fig['excluded_share'] <= 0.01
    assert fig['hit_miss_mismatches'] == 0
    assert fig['max_abs_depth_err'] <= DEPTH_BAR


def test_transform_and_backface_culling():
    """The per-call rigid transform equals transforming the vertices first (a quarter turn, which is exact, so bit for
    bit; the tool's test adds an exact translation), and the cull flag keeps the side whose vertices run counter-clockwise as seen from the camera."""
    occ = _occ()
    v, f = rr.uv_sphere(16, 32, 0.5, (0.0, 0.0, 3.0))
    m = np.array([[0, -1, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float64)
    v2 = (v.astype(np.float64) @ m[:3, :3].T + m[:3, 3]).astype(np.float32)
    a = occ.depth_render(_dev(v), f, CAM, SIZE, transform=m)
    b = occ.depth_render(_dev(v2), f, CAM, SIZE)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    two = occ.depth_render(_dev(v2), f, CAM, SIZE)[0].cpu().numpy()
    for faces in (f, f[:, ::-1].copy()):
        got = occ.depth_render(_dev(v2), faces, CAM, SIZE, cull_backfaces=True)[0].cpu().numpy().astype(np.float64)
        ref, edge = rr.render(v2, faces, CAM, SIZE, cull_backfaces=True, with_edges=True)
        clear = edge >= EDGE_BAND
        assert ((got > 0) == (ref > 0))[clear].all()
        assert np.abs(got - ref)[clear & (ref > 0)].max() <= DEPTH_BAR
    near = occ.depth_render(_dev(v2), f, CAM, SIZE, cull_backfaces=True)[0].cpu().numpy()
    far = occ.depth_render(_dev(v2), f[:, ::-1].copy(), CAM, SIZE, cull_backfaces=True)[0].cpu().numpy()
    hit = two > 0
    assert hit.sum() > 10000
    front, back = (near, far) if near[hit].mean() < far[hit].mean() else (far, near)
    assert (np.minimum(np.where(front > 0, front, np.inf), np.where(back > 0, back, np.inf))[hit] == two[hit]).all()


@pytest.mark.parametrize('name', ['sphere', 'field', 'box'])
def test_probe_equals_render_bit_for_bit(name):
    occ = _occ()
    v, f = MESHES[name]()
    g = np.random.Generator(np.random.PCG64(11))
    P = 10000
    pix = np.stack([g.integers(-60, W + 60, P), g.integers(-60, H + 60, P)], -1).astype(np.int32)
    if name != 'box':          # the sphere covers little of the image: put half of the pixels where it is
        pix[:P // 2] = np.stack([g.integers(700, 1200, P // 2), g.integers(300, 780, P // 2)], -1)
    img = occ.depth_render(_dev(v), f, CAM, SIZE)[0]
    got = occ.depth_probe(_dev(v), f, _dev(pix)[None], CAM, SIZE)[0]
    inside = (pix[:, 0] >= 0) & (pix[:, 0] < W) & (pix[:, 1] >= 0) & (pix[:, 1] < H)
    assert (~inside).sum() > 200
    want = torch.zeros(P, dtype=torch.float32, device=DEV)
    ins = _dev(inside)
    px = _dev(pix).long()
    want[ins] = img[px[ins, 1], px[ins, 0]]
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert int((got > 0).sum()) > 1000
    assert float(got[~ins].abs().max()) == 0.0


# ---- bodies ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def world(tmp_path_factory):
    """Everything tests 4-6 share: the body model (through an SMPLX_NEUTRAL.npz, as the tool loads it), 64 posed frames,
    the device's vertices / joints copied back, device and restatement renders, and the per-frame comparison figures."""
    from rohm_amd.body_model import SMPLXLayer, lbs_forward, native_for
    occ = _occ()
    root = tmp_path_factory.mktemp('occlusion')
    tensors, faces = sphere_body()
    npz = str(root / 'SMPLX_NEUTRAL.npz')
    write_npz(npz, tensors, faces)
    body = SMPLXLayer.from_npz(npz).to(DEV)
    assert body.faces is not None
    params = walking_params(tensors)
    nat = native_for(body, torch.device(DEV))
    pose = torch.cat([_dev(params['global_orient']).reshape(N_FRAMES, 1, 3), _dev(params['body_pose']).reshape(N_FRAMES, 21, 3)], 1)
    joints, verts = lbs_forward(nat, pose.contiguous(), 0, _dev(params['betas']), _dev(params['transl']))
    sv, sf = scene_mesh()
    scene_gpu = occ.depth_render(_dev(sv), sf, CAM, SIZE)[0]
    bodies_gpu = occ.depth_render(verts, faces, CAM, SIZE)
    mask_gpu = occ.joint_occlusion_mask(body, {k: _dev(v) for k, v in params.items()}, scene_gpu, CAM, DIST, thr=0.1,
                                        proj_camera_mtx=K_COLOR)
    v_host, j_host = verts.cpu().numpy(), joints[:, :25].cpu().numpy()
    scene_ref, scene_edge = rr.render(sv, sf, CAM, SIZE, with_edges=True)
    uv = rr.project(j_host, K_COLOR, DIST)
    pix = rr.to_pixels(uv)
    inside = (pix[..., 0] >= 0) & (pix[..., 0] < W) & (pix[..., 1] >= 0) & (pix[..., 1] < H)
    xs, ys = np.clip(pix[..., 0], 0, W - 1), np.clip(pix[..., 1], 0, H - 1)
    body_at = np.zeros((N_FRAMES, 25))
    edge_at = np.full((N_FRAMES, 25), np.inf)
    figs = []
    for i in range(N_FRAMES):
        ref, edge = rr.render(v_host[i], faces, CAM, SIZE, with_edges=True)
        figs.append(_compare(bodies_gpu[i].cpu().numpy(), ref, edge))
        body_at[i] = ref[ys[i], xs[i]]
        edge_at[i] = np.minimum(edge[ys[i], xs[i]], scene_edge[ys[i], xs[i]])
    return dict(root=root, npz=npz, body=body, faces=faces, params=params, verts=verts, scene=(sv, sf), scene_gpu=scene_gpu,
                bodies_gpu=bodies_gpu, mask_gpu=mask_gpu.cpu().numpy(), scene_ref=scene_ref, uv=uv, pix=pix, inside=inside,
                body_at=body_at, edge_at=edge_at, figs=figs, joints=j_host)


def test_render_is_bitwise_reproducible(world):
    occ = _occ()
    again = occ.depth_render(world['verts'], world['faces'], CAM, SIZE)
    assert torch.equal(again.view(torch.int32), world['bodies_gpu'].view(torch.int32))
    v, f = MESHES['field']()
    a, b = occ.depth_render(_dev(v), f, CAM, SIZE), occ.depth_render(_dev(v), f, CAM, SIZE)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_batched_bodies_match_restatement(world):
    """64 LBS bodies in one call; the restatement is fed the device's own vertices, so only the renderer is judged."""
    figs = world['figs']
    covered = sum(f['covered'] for f in figs)
    excluded = sum(f['excluded'] for f in figs)
    fig = {'frames': len(figs), 'covered': covered, 'excluded_share': excluded / max(1, covered),
           'hit_miss_mismatches': sum(f['hit_miss_mismatches'] for f in figs),
           'max_abs_depth_err': max(f['max_abs_depth_err'] for f in figs)}
    print(fig)
    _record('depth_bodies', fig)
    assert sum(f['covered'] > 5000 for f in figs) >= 40          # some frames have walked out of view
    assert fig['excluded_share'] <= 0.01
    assert fig['hit_miss_mismatches'] == 0
    assert fig['max_abs_depth_err'] <= DEPTH_BAR
    # the probe on the batch: bit for bit the rendered images
    g = np.random.Generator(np.random.PCG64(2))
    P = 2000
    pix = np.stack([g.integers(-20, W + 20, (N_FRAMES, P)), g.integers(-20, H + 20, (N_FRAMES, P))], -1).astype(np.int32)
    pix[:, :P // 2] = (world['pix'][:, :1, :] + g.integers(-150, 150, (N_FRAMES, P // 2, 2))).clip(-5, 4000)
    got = _occ().depth_probe(world['verts'], world['faces'], _dev(pix), CAM, SIZE)
    px = _dev(pix).long()
    ins = (px[..., 0] >= 0) & (px[..., 0] < W) & (px[..., 1] >= 0) & (px[..., 1] < H)
    idx = torch.arange(N_FRAMES, device=DEV)[:, None].expand(-1, P)
    want = torch.where(ins, world['bodies_gpu'][idx, px[..., 1].clamp(0, H - 1), px[..., 0].clamp(0, W - 1)],
                       torch.zeros((), device=DEV))
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert int((got > 0).sum()) > 5000


def test_masks_end_to_end(world):
    ref_mask, margin = rr.occlusion_mask(world['pix'], world['scene_ref'], world['body_at'], 0.1)
    gpu = world['mask_gpu']
    assert gpu.shape == (N_FRAMES, 25) and gpu.dtype == np.float32
    frac = np.abs(world['uv'] - np.round(world['uv'])).min(-1)
    inside = world['inside']
    scene_at = np.where(inside, world['scene_ref'][np.clip(world['pix'][..., 1], 0, H - 1), np.clip(world['pix'][..., 0], 0, W - 1)], 0.0)
    excluded = (frac < 1e-3) | (inside & ((np.abs(margin) < 1e-3) | (world['edge_at'] < EDGE_BAND)))
    share = float(excluded.mean())
    fig = {'pairs': int(gpu.size), 'excluded_share': share, 'occluded': int((gpu == 0).sum()),
           'outside_image': int((~inside).sum()), 'scene_empty': int((inside & (scene_at == 0)).sum()),
           'mismatches': int(((gpu != ref_mask) & ~excluded).sum())}
    print(fig)
    _record('mask', fig)
    assert share <= 0.02
    assert fig['mismatches'] == 0
    assert (gpu == 0).sum() > 50 and (gpu == 1).sum() > 50
    assert set(np.unique(gpu).tolist()) == {0.0, 1.0}
    assert (~inside).sum() > 20 and (gpu[~inside] == 1).all()
    empty = inside & (scene_at == 0) & ~excluded
    assert empty.sum() > 20 and (gpu[empty] == 1).all()


def test_mask_pieces_follow_the_decision(world):
    """rohm_project_pixels and rohm_joint_occlusion_mask on hand-made depths: every branch of :138-143."""
    occ = _occ()
    joints = _dev(world['joints'])
    pix = occ.project_pixels(joints, K_COLOR, DIST).cpu().numpy()
    uv = world['uv']
    frac = np.abs(uv - np.round(uv)).min(-1)
    ok = frac > 1e-6
    assert (pix[ok] == world['pix'][ok]).all()
    neg = np.array([[[-0.0007, -0.0004, 1.0], [0.0, 0.0, 0.0], [1e30, 0.0, 1e-30]]], dtype=np.float32)
    p = occ.project_pixels(_dev(neg), K_COLOR, None).cpu().numpy()[0]
    assert p[0].tolist() == [950, 536]                      # 950.56 -> 950, 536.35 -> 536 (toward zero)
    assert p[1].tolist() == [951, 536]                      # z == 0 divides by 1
    assert p[2, 0] < 0                                      # beyond the int range: outside every image
    scene = torch.zeros(H, W, device=DEV)
    scene[536, 950] = 2.0
    j = np.tile(neg[:, :1], (1, 4, 1))
    body = _dev(np.array([[2.2, 2.05, 0.0, 2.1000004]], dtype=np.float32))
    m = occ.mask_from_depths(_dev(j), scene, body, K_COLOR, None, thr=0.1).cpu().numpy()[0]
    assert m.tolist() == [0.0, 1.0, 1.0, float(np.float32(2.1000004) - np.float32(2.0) <= np.float32(0.1))]
    scene[536, 950] = 0.0
    assert occ.mask_from_depths(_dev(j), scene, body, K_COLOR, None, thr=0.1).cpu().numpy().tolist() == [[1.0] * 4]


def test_cli_writes_the_mask_file(world, tmp_path):
    """A synthetic PROX tree, one child process; the file has the script's shape and dtype and test 5's values."""
    scene, seq = 'TestRoom', 'TestRoom_00001_01'
    prox = tmp_path / 'PROX'
    for d in ('scenes', 'cam2world', 'calibration'):
        (prox / d).mkdir(parents=True)
    # an exactly representable rigid transform: the scene file is in world coordinates, the tool maps it back
    c2w = np.array([[0, 0, 1, 1.5], [-1, 0, 0, -0.25], [0, -1, 0, 2.0], [0, 0, 0, 1]], dtype=np.float64)
    sv, sf = world['scene']
    wv = (sv.astype(np.float64) @ c2w[:3, :3].T + c2w[:3, 3]).astype(np.float32)
    back = wv.astype(np.float64) @ np.linalg.inv(c2w)[:3, :3].T + np.linalg.inv(c2w)[:3, 3]
    assert np.array_equal(back.astype(np.float32), sv)
    head = ['ply', 'format binary_little_endian 1.0', f'element vertex {len(wv)}', 'property float x', 'property float y',
            'property float z', 'property uchar red', 'property uchar green', 'property uchar blue', f'element face {len(sf)}',
            'property list uchar int vertex_indices', 'end_header']
    blob = ('\n'.join(head) + '\n').encode()
    for p in wv:
        blob += np.asarray(p, '<f4').tobytes() + bytes([200, 200, 200])
    for t in sf:
        blob += bytes([3]) + np.asarray(t, '<i4').tobytes()
    (prox / 'scenes' / (scene + '.ply')).write_bytes(blob)
    (prox / 'cam2world' / (scene + '.json')).write_text(json.dumps(c2w.tolist()))
    (prox / 'calibration' / 'Color.json').write_text(json.dumps({'camera_mtx': K_COLOR, 'k': DIST, 'f': [1060.53, 1060.38],
                                                                 'c': [951.30, 536.77]}))
    init = tmp_path / 'init_prox_rgbd'
    for i in range(N_FRAMES):
        d = init / seq / 'results' / f's001_frame_{i + 1:05d}__00.00.00.{i:03d}'
        d.mkdir(parents=True)
        with open(d / '000.pkl', 'wb') as f:
            pickle.dump({k: v[i:i + 1] for k, v in world['params'].items()}, f)
    models = tmp_path / 'smplx_model' / 'smplx'
    models.mkdir(parents=True)
    with open(world['npz'], 'rb') as src:
        (models / 'SMPLX_NEUTRAL.npz').write_bytes(src.read())
    out = tmp_path / 'mask_joint_prox'
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'rohm_amd.occlusion', '--prox_root', str(prox), '--body_model_path',
                        str(tmp_path / 'smplx_model'), '--init_body_path', str(init), '--save_mask_path', str(out),
                        '--scene_name', scene, '--seq_name', seq], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    m = np.load(out / seq / 'mask_joint.npy')
    assert m.shape == (N_FRAMES, 25) and m.dtype == np.float64
    assert np.array_equal(m, world['mask_gpu'].astype(np.float64))
    # the reference's img_list[0:100] cut, in process
    assert _occ().main(['--prox_root', str(prox), '--body_model_path', str(tmp_path / 'smplx_model'), '--init_body_path', str(init),
                        '--save_mask_path', str(out), '--scene_name', scene, '--seq_name', seq, '--max_frames', '10']) == 0
    assert np.array_equal(np.load(out / seq / 'mask_joint.npy'), world['mask_gpu'][:10].astype(np.float64))
