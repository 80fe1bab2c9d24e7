"""GPU: the export step -- `rohm_export_smplx` (csrc/export.hip) against its float64 restatement (tests/export_ref.py, itself
pinned to the reference by tests/golden/export.npz), the skinned consistency of the exported parameters, the round trip
through the native loader, the closed loop export -> fits -> loader, and the command line.

Kernel and restatement are both float64 on the same float32 inputs and differ by libm and fma contraction only: the bar is
1e-9 absolute on all 79 columns.  The measured maxima go to profiles/export_parity.json."""
import json
import math
import os
import pickle

import numpy as np
import pytest
import torch

import export_ref as ER
import video_tree as VT
from helpers import golden
from rohm_amd.utils import synth

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_BAR = 1e-9
GEOM_TOL = 5e-6                       # tests/test_gpu_video_loader.py: its bar for `noisy_joints_scene_coord`
LBS_VERT_BAR, LBS_JOINT_BAR = 2e-5, 1e-5          # tests/test_gpu_rederive.py::test_lbs_skinning_paths_vs_oracle
PARITY = {}


def _record(key, value):
    path = os.path.join(ROOT, 'profiles', 'export_parity.json')
    PARITY[key] = max(float(value), PARITY.get(key, 0.0))
    try:
        with open(path) as f:
            data = json.load(f)
    except (OSError, ValueError):
        data = {}
    data.setdefault('gpu', {}).update(PARITY)
    try:
        with open(path, 'w') as f:
            json.dump(data, f, indent=1, sort_keys=True)
            f.write('\n')
    except OSError:
        pass


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _layer(tensors):
    from rohm_amd.body_model import SMPLXLayer
    return SMPLXLayer.from_tensors(tensors).to(DEV)


@pytest.fixture(scope='module')
def small():
    """The fixture's clips (C = 3, T = 7, de-normalised), a normalised copy, and the 419-vertex synthetic body model."""
    from rohm_amd.body_model import native_for
    g = golden('export.npz')
    tensors = synth.synthetic_smplx_tensors(0, num_verts=int(g['num_verts']))
    layer = _layer(tensors)
    mean, std = synth.synthetic_stats(3)
    rep = g['repr'].astype(np.float32)
    cam2world = np.eye(4)
    cam2world[:3, :3] = ER.rodrigues(np.array([0.25, -0.5, 0.15]))
    cam2world[:3, 3] = [0.4, -1.1, 2.2]
    return {'g': g, 'tensors': tensors, 'layer': layer, 'handle': native_for(layer, torch.device(DEV)).handle,
            'pelvis': ER.fold_pelvis(tensors), 'rep': rep, 'rep_norm': ((rep - mean) / std).astype(np.float32), 'mean': mean, 'std': std,
            'transf': g['transf'].astype(np.float32), 'rigid': np.linalg.inv(cam2world), 'cam2world': cam2world}


def _launch(s, rep, layout, fc, ft, stats, transf, rigid):
    from rohm_amd import ops
    x = _dev(rep)
    if layout == 'bc1t':
        x = x.permute(0, 2, 1).unsqueeze(2).contiguous()          # [C, 294, 1, T]
    return ops.export_smplx(s['handle'], x, layout, _dev(fc, torch.int32), _dev(ft, torch.int32),
                            transf=_dev(s['transf'][:rep.shape[0]]) if transf else None, rigid=_dev(s['rigid']) if rigid else None,
                            mean=_dev(s['mean']) if stats else None, std=_dev(s['std']) if stats else None)


def _restate(s, rep, fc, ft, stats, transf, rigid):
    return ER.export_params(rep, fc, ft, s['pelvis'], transf=s['transf'] if transf else None, rigid=s['rigid'] if rigid else None,
                            mean=s['mean'] if stats else None, std=s['std'] if stats else None)


# ---- kernel against restatement --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('keep', ['first', 'last'])
@pytest.mark.parametrize('rigid', [False, True])
@pytest.mark.parametrize('transf', [False, True])
@pytest.mark.parametrize('stats', [False, True])
@pytest.mark.parametrize('layout', ['btc', 'bc1t'])
def test_kernel_matches_the_restatement(small, layout, stats, transf, rigid, keep):
    from rohm_amd.export import plan_frames
    rep = small['rep_norm'] if stats else small['rep']
    fc, ft, n = plan_frames(3, 7, 8, 2, keep)
    assert n == 19
    params, contact = _launch(small, rep, layout, fc, ft, stats, transf, rigid)
    assert tuple(params.shape) == (19, 79) and params.dtype == torch.float64
    assert tuple(contact.shape) == (19, 4) and contact.dtype == torch.float32
    want, want_contact = _restate(small, rep, fc, ft, stats, transf, rigid)
    err = np.abs(params.cpu().numpy() - want).max()
    print(f'{layout} stats={stats} transf={transf} rigid={rigid} keep={keep}: max |kernel - restatement| = {err:.3e}')
    _record('kernel_vs_restatement_max_abs', err)
    assert err <= KERNEL_BAR
    assert np.array_equal(contact.cpu().numpy(), want_contact)          # the same two float32 operations
    again, _ = _launch(small, rep, layout, fc, ft, stats, transf, rigid)
    assert torch.equal(again, params)                                   # no atomics: the same input gives the same bits
    ang = params[:, :3].norm(dim=1)
    assert float(ang.max()) <= math.pi


def test_out_of_range_index_gives_a_nan_row_and_touches_nothing_else(small):
    from rohm_amd.export import plan_frames
    fc, ft, _ = plan_frames(3, 7, 8, 2)
    good, good_contact = _launch(small, small['rep_norm'], 'bc1t', fc, ft, True, True, True)
    bad_c, bad_t = fc.copy(), ft.copy()
    bad = {2: (3, 0), 5: (-1, 3), 9: (1, 7), 17: (2, -1), 18: (2 ** 31 - 1, 2 ** 31 - 1)}
    for n, (c, t) in bad.items():
        bad_c[n], bad_t[n] = c, t
    got, contact = _launch(small, small['rep_norm'], 'bc1t', bad_c, bad_t, True, True, True)
    rows = sorted(bad)
    rest = [n for n in range(19) if n not in bad]
    assert torch.isnan(got[rows]).all() and torch.isnan(contact[rows]).all()
    assert torch.equal(got[rest], good[rest]) and torch.equal(contact[rest], good_contact[rest])
    want, _ = _restate(small, small['rep_norm'], bad_c, bad_t, True, True, True)
    assert np.array_equal(np.isnan(got.cpu().numpy()), np.isnan(want))


def test_no_frames_no_launch(small):
    from rohm_amd import ops
    from rohm_amd._lib import RohmHipError
    from rohm_amd.export import export_params
    empty = np.zeros(0, np.int32)
    params, contact = _launch(small, small['rep'], 'btc', empty, empty, False, True, False)
    assert tuple(params.shape) == (0, 79) and tuple(contact.shape) == (0, 4)
    res = export_params(np.zeros((0, 7, 294), np.float32), np.zeros((0, 4, 4), np.float32), small['layer'], clip_len=8)
    assert len(res) == 0 and tuple(res.joints.shape) == (0, 22, 3)
    with pytest.raises(RohmHipError):
        ops.export_smplx(small['handle'], torch.zeros(3, 7, 294), 'btc', torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.export_smplx(small['handle'], _dev(small['rep']), 'btc', _dev(empty), _dev(empty), mean=_dev(small['mean']))


def test_hand_made_rotations(small):
    """The identity, angle 1e-7, angle pi - 1e-4 and a non-unit, non-orthogonal 6-D vector, as root and as body rotations."""
    rows6, axis = ER.hard_rotations()
    rep = np.zeros((1, 4, 294), np.float32)
    rep[0, :, 280:290] = small['rep'][0, :4, 280:290]
    rep[0, :, 16:19] = small['rep'][0, :4, 16:19]
    for t in range(4):
        rep[0, t, 7:13] = rows6[t]
        for j in range(21):
            rep[0, t, 154 + j * 6:160 + j * 6] = rows6[(t + j + 1) % 4]
    fc, ft = np.zeros(4, np.int32), np.arange(4, dtype=np.int32)
    for transf, rigid in ((False, False), (True, True)):
        got = _launch(small, rep, 'btc', fc, ft, False, transf, rigid)[0].cpu().numpy()
        want = _restate(small, rep, fc, ft, False, transf, rigid)[0]
        rv = lambda p: np.concatenate([p[:, 0:3].reshape(-1, 1, 3), p[:, 16:79].reshape(-1, 21, 3)], axis=1)
        g_rv, w_rv = rv(got), rv(want)
        near_pi = np.linalg.norm(w_rv, axis=-1) > math.pi - 1e-3
        assert near_pi.sum() >= 21
        err_mat = np.abs(ER.rodrigues(g_rv) - ER.rodrigues(w_rv)).max()
        err_vec = np.abs(g_rv - w_rv)[~near_pi].max()
        err_rest = max(np.abs(got[:, 3:16] - want[:, 3:16]).max(), err_vec)
        print(f'hand-made rotations transf={transf}: matrices {err_mat:.3e}, vectors away from pi {err_vec:.3e}, '
              f'vectors near pi {np.abs(g_rv - w_rv)[near_pi].max():.3e}')
        _record('hand_made_rotations_max_abs', max(err_mat, err_rest))
        assert err_mat <= KERNEL_BAR and err_rest <= KERNEL_BAR
        assert np.linalg.norm(g_rv, axis=-1).max() <= math.pi
    # without a transform the root rows are the rotations themselves: zero, 1e-7 (not kornia's 2 v), pi - 1e-4
    got = _launch(small, rep, 'btc', fc, ft, False, False, False)[0].cpu().numpy()
    assert np.array_equal(got[0, 0:3], np.zeros(3))
    assert np.abs(got[1, 0:3] - axis * 1e-7).max() < 1e-13
    assert abs(np.linalg.norm(got[2, 0:3]) - (math.pi - 1e-4)) < 1e-6


# ---- skinned consistency ---------------------------------------------------------------------------------------------------
def test_skinning_the_exported_parameters_is_the_transformed_canonical_body(small):
    """rohm_smplx_forward(exported axis-angle parameters) == A . rohm_smplx_forward(canonical 6-D pose).  Two skinning
    evaluations are compared, so the bar is twice that of tests/test_gpu_rederive.py::test_lbs_skinning_paths_vs_oracle
    (vertices 2e-5, joints 1e-5 against its oracle)."""
    from rohm_amd.body_model import lbs_forward, native_for
    from rohm_amd.export import export_params, export_vertices
    nat = native_for(small['layer'], torch.device(DEV))
    rep = small['rep']
    C, T = rep.shape[:2]
    plan = (np.repeat(np.arange(C), T).astype(np.int32), np.tile(np.arange(T), C).astype(np.int32))
    rows = _dev(rep.reshape(C * T, 294))
    pose6 = torch.cat([rows[:, 7:13], rows[:, 154:280]], dim=1).reshape(C * T, 22, 6).contiguous()
    j_cano, v_cano = lbs_forward(nat, pose6, 1, rows[:, 280:290].contiguous(), rows[:, 16:19].contiguous())
    for frame, cam2world in (('scene', None), ('camera', small['cam2world'])):
        res = export_params(rep, small['transf'], small['layer'], frame=frame, cam2world=cam2world, plan=plan)
        verts = export_vertices(res, small['layer'], chunk=8)
        assert tuple(verts.shape) == (C * T, int(small['g']['num_verts']), 3)
        A = np.stack([ER.affine(small['transf'][c], small['rigid'] if frame == 'camera' else None) for c in plan[0]])
        move = lambda p: np.einsum('nij,nvj->nvi', A[:, :3, :3], p.double().cpu().numpy()) + A[:, None, :3, 3]
        err_v = np.abs(verts.cpu().numpy() - move(v_cano)).max()
        err_j = np.abs(res.joints.cpu().numpy() - move(j_cano[:, :22])).max()
        print(f'skinned consistency ({frame}): vertices {err_v:.3e}, joints {err_j:.3e}')
        _record(f'skinned_consistency_{frame}_vertices', err_v)
        assert err_v <= 2 * LBS_VERT_BAR and err_j <= 2 * LBS_JOINT_BAR
        assert tuple(export_vertices(res, small['layer'], every=4).shape) == (6, int(small['g']['num_verts']), 3)
    # the scene vertices are the reference's (points_coord_trans of its canonical vertices), to float32 skinning accuracy
    res = export_params(rep, small['transf'], small['layer'], frame='scene', plan=plan)
    verts = export_vertices(res, small['layer'])[:, _dev(small['g']['vert_index'])].cpu().numpy()
    assert np.abs(verts - small['g']['scene_verts']).max() <= 2 * LBS_VERT_BAR


# ---- the native loader: round trip and closed loop -------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def big():
    tensors = synth.synthetic_smplx_tensors(0)
    return tensors, _layer(tensors)


@pytest.fixture(scope='module')
def cpu_round_trip(big):
    from rohm_amd.export import plan_frames
    return ER.roundtrip_cpu(golden('video_loader.npz'), big[0], plan_frames)


def _tree(tmp, dataset):
    a = VT.tree_arrays_from_fixture(golden('video_loader.npz'), dataset)
    return a, VT.write_tree(str(tmp), dataset, a)


def _loader(a, paths, dataset, layer):
    from rohm_amd.data_loaders.dataloader_video import DataloaderVideo
    return DataloaderVideo(dataset=dataset, init_root=paths['init_root'], base_dir=paths['base_dir'], body_model_path=layer,
                           recording_name=str(a['recording_name']), use_scene_floor_height=False, repr_abs_only=False, task='pose',
                           overlap_len=VT.OVERLAP, clip_len=VT.CLIP_LEN, logdir=paths['logdir'], device=DEV)


@pytest.fixture(scope='module')
def loaders(big, tmp_path_factory):
    out = {}
    for dataset in ('prox', 'egobody'):
        a, paths = _tree(tmp_path_factory.mktemp(dataset), dataset)
        ds = _loader(a, paths, dataset, big[1])
        out[dataset] = (a, paths, ds, next(ds.batches(3)))
    return out


@pytest.mark.parametrize('dataset', ['prox', 'egobody'])
def test_loader_round_trip_reproduces_the_world_parameters(big, loaders, cpu_round_trip, dataset):
    from rohm_amd.export import export_params
    a, _, ds, batch = loaders[dataset]
    assert tuple(batch['motion_repr_noisy'].shape) == (3, 7, 294)
    world, _ = ER.world_params_of_tree(a, dataset, big[0])
    bar = 4 * cpu_round_trip['roundtrip_cpu_error']
    for keep in ('first', 'last'):
        res = export_params(batch['motion_repr_noisy'], batch['transf_matrix'], big[1], clip_len=VT.CLIP_LEN, overlap_len=VT.OVERLAP,
                            frame='scene', stats=ds, keep=keep)
        assert len(res) == 19 and res.coordinate_frame == 'scene'
        rot, tr, betas = ER.param_errors(res.params79.cpu().numpy(), world[:19])
        print(f'{dataset} keep={keep}: rotation matrices {rot:.3e}, translation {tr:.3e}, betas {betas:.3e}; bar {bar:.3e} '
              f"(CPU: {cpu_round_trip[dataset]})")
        _record(f'loader_round_trip_{dataset}', max(rot, tr))
        assert rot <= bar and tr <= bar and betas <= 1e-6
    # the network's layout, read in place
    x = batch['motion_repr_noisy'].permute(0, 2, 1).unsqueeze(2).contiguous()
    res2 = export_params(x, batch['transf_matrix'], big[1], clip_len=VT.CLIP_LEN, overlap_len=VT.OVERLAP, stats=ds, keep='last')
    assert torch.equal(res2.params79, res.params79) and torch.equal(res2.joints, res.joints)


@pytest.mark.parametrize('dataset', ['prox', 'egobody'])
def test_closed_loop_export_fits_loader(big, loaders, tmp_path, dataset):
    """export (camera frame) -> write_prox_fits into a copy of the tree -> a second loader: its scene-frame joints are the
    export's scene-frame joints on the 19 covered frames."""
    from rohm_amd.data_loaders.dataloader_video import read_cam2world
    from rohm_amd.export import export_params, write_prox_fits
    a, paths, ds, batch = loaders[dataset]
    rec = str(a['recording_name'])
    kw = dict(clip_len=VT.CLIP_LEN, overlap_len=VT.OVERLAP, stats=ds)
    scene = export_params(batch['motion_repr_noisy'], batch['transf_matrix'], big[1], frame='scene', **kw)
    cam = export_params(batch['motion_repr_noisy'], batch['transf_matrix'], big[1], frame='camera',
                        cam2world=read_cam2world(dataset, paths['base_dir'], rec), **kw)
    assert cam.coordinate_frame == 'camera' and torch.equal(cam.betas, scene.betas) and torch.equal(cam.body_pose, scene.body_pose)
    _, paths2 = _tree(tmp_path, dataset)
    names = [str(s) for s in a['frame_names']]
    write_prox_fits(paths2['init_root'], rec, cam, names, body_idx=int(a['target_idx']) if dataset == 'egobody' else None)
    ds2 = _loader(a, paths2, dataset, big[1])
    assert len(ds2) == 3
    jw = next(ds2.batches(3))['noisy_joints_scene_coord']          # [3, 8, 22, 3]: clips start at frames 0, 6, 12
    stride = VT.CLIP_LEN - VT.OVERLAP
    per_frame = torch.stack([jw[min(f // stride, 2), f - min(f // stride, 2) * stride] for f in range(19)])
    err = float((per_frame - scene.joints).abs().max())
    print(f'{dataset}: closed loop max |loader joints - exported joints| = {err:.3e}')
    _record(f'closed_loop_{dataset}', err)
    assert err <= GEOM_TOL
    # frame 19 was not exported: its fit is still the tree's, so the loop did go through the written files
    assert float((jw[2, 7] - loaders[dataset][3]['noisy_joints_scene_coord'][2, 7]).abs().max()) == 0.0
    assert float((per_frame - torch.stack([loaders[dataset][3]['noisy_joints_scene_coord'][min(f // stride, 2), f - min(f // stride, 2) * stride]
                                           for f in range(19)])).abs().max()) <= 2 * GEOM_TOL


def test_mean_betas_are_consistent(big, loaders):
    """betas='mean': one shape for the whole track, with the pelvis offset and the translation made for it -- consistency of
    the export with itself, not parity with the reference (which keeps per-frame shapes)."""
    from rohm_amd.data_loaders.frames import noisy_clip_joints
    from rohm_amd.export import export_params, plan_frames
    a, paths, ds, batch = loaders['prox']
    x = batch['motion_repr_noisy'].clone()
    x[:, :, 280:290] += 0.3 * torch.randn(x[:, :, 280:290].shape, generator=torch.Generator().manual_seed(4)).to(DEV)
    x0 = x.clone()
    kw = dict(clip_len=VT.CLIP_LEN, overlap_len=VT.OVERLAP, stats=ds, frame='scene')
    per_frame = export_params(x, batch['transf_matrix'], big[1], **kw)
    res = export_params(x, batch['transf_matrix'], big[1], betas='mean', **kw)
    assert float((res.betas - res.betas[:1]).abs().max()) == 0.0
    assert float((res.betas[0] - per_frame.betas.mean(dim=0)).abs().max()) < 1e-6
    assert float(per_frame.betas.std(dim=0).max()) > 0.05
    assert torch.equal(res.global_orient, per_frame.global_orient) and torch.equal(res.body_pose, per_frame.body_pose)
    written = {k: getattr(res, k).float() for k in ('global_orient', 'transl', 'betas', 'body_pose')}
    assert torch.equal(res.joints, noisy_clip_joints(big[1], written, DEV))
    # the restatement fed with that shape gives the same rows
    mean, std = ds.Mean.astype(np.float32), ds.Std.astype(np.float32)
    den = x.cpu().numpy() * std + mean
    den[:, :, 280:290] = res.betas[0].float().cpu().numpy()
    fc, ft, _ = plan_frames(3, 7, VT.CLIP_LEN, VT.OVERLAP)
    want, _ = ER.export_params(den, fc, ft, ER.fold_pelvis(big[0]), transf=batch['transf_matrix'].cpu().numpy())
    assert np.abs(res.params79.cpu().numpy() - want).max() <= KERNEL_BAR
    assert torch.equal(x, x0) and not torch.equal(res.transl, per_frame.transl)          # the caller's tensor is not written


# ---- the command line --------------------------------------------------------------------------------------------------------
def test_command_line(small, loaders, tmp_path, capsys):
    from raster_scenes import write_npz as write_body_npz
    from rohm_amd import export as E
    from rohm_amd.drivers.results import result_rows
    from rohm_amd.occlusion import read_ply
    a, paths, ds, batch = loaders['prox']
    rec = str(a['recording_name'])
    den = result_rows([(batch['motion_repr_noisy'], 'btc')], ds)[0].cpu().numpy()
    transf = batch['transf_matrix'].cpu().numpy()
    # 3 clips in batches of 3: the drivers' loop runs batch 0 twice
    save = {'repr_name_list': [], 'motion_repr_rec_list': np.concatenate([den, den]), 'trans_scene2cano_list': np.concatenate([transf, transf]),
            'frame_name_list': np.array([['x'] * 8] * 3), 'recording_name': rec}
    pkl_dir = tmp_path / 'results'
    pkl_dir.mkdir()
    with open(pkl_dir / (rec + '.pkl'), 'wb') as f:
        pickle.dump(save, f, protocol=2)
    V = int(small['g']['num_verts'])
    faces = np.random.Generator(np.random.PCG64(2)).integers(0, V, size=(64, 3))
    body_npz = str(tmp_path / 'SMPLX_NEUTRAL.npz')
    write_body_npz(body_npz, small['tensors'], faces)
    out = tmp_path / 'out'
    interval = 4
    rc = E.main(['--dataset', 'prox', '--saved_data_dir', str(pkl_dir), '--recordings', rec, '--dataset_root', paths['base_dir'],
                 '--body_model_path', body_npz, '--out', str(out), '--frame', 'camera', '--formats', 'npz,prox_fits', '--meshes', 'ply',
                 '--mesh_interval', str(interval), '--init_root', paths['init_root'], '--device', DEV])
    assert rc == 0
    text = capsys.readouterr().out
    assert 'rows 3..5 repeat the first batch, dropped' in text and '19 frames exported' in text
    names = [str(s) for s in a['frame_names']][:19]
    d = np.load(str(out / rec / 'smplx_params.npz'))
    assert d['frame_names'].tolist() == names and str(d['coordinate_frame']) == 'camera' and d['transl'].shape == (19, 3)
    fits = out / rec / 'fits' / rec / 'results'
    assert sorted(os.listdir(fits)) == names
    meshes = sorted(os.listdir(out / rec / 'meshes'))
    assert meshes == sorted(n + '.ply' for n in names[::interval]) and len(meshes) == math.ceil(19 / interval)
    for m in meshes:
        v, f = read_ply(str(out / rec / 'meshes' / m))
        assert v.shape == (V, 3) and np.array_equal(f, faces)
    # the files hold what export_params returns for the same inputs
    from rohm_amd.body_model import SMPLXLayer
    from rohm_amd.data_loaders.dataloader_video import read_cam2world, read_fittings
    layer = SMPLXLayer.from_npz(body_npz).to(DEV)
    res = E.export_params(den, transf, layer, clip_len=VT.CLIP_LEN, overlap_len=VT.OVERLAP, frame='camera',
                          cam2world=read_cam2world('prox', paths['base_dir'], rec))
    assert np.array_equal(d['global_orient'], res.global_orient.float().cpu().numpy())
    assert np.array_equal(read_fittings(str(fits), names)['transl'], res.transl.float().cpu().numpy())
    v, _ = read_ply(str(out / rec / 'meshes' / meshes[1]))
    assert np.array_equal(v, E.export_vertices(res, layer, every=interval)[1].cpu().numpy())
    # AMASS pickles: every clip is its own sequence, in its canonical frame
    with open(tmp_path / 'amass.pkl', 'wb') as f:
        pickle.dump({'motion_repr_rec_list': den[:2]}, f, protocol=2)
    assert E.main(['--dataset', 'amass', '--saved_data_path', str(tmp_path / 'amass.pkl'), '--body_model_path', body_npz,
                   '--out', str(tmp_path / 'amass_out'), '--device', DEV]) == 0
    seqs = sorted(os.listdir(tmp_path / 'amass_out' / 'amass'))
    assert seqs == ['seq_000', 'seq_001']
    d = np.load(str(tmp_path / 'amass_out' / 'amass' / 'seq_001' / 'smplx_params.npz'))
    assert d['transl'].shape == (7, 3) and d['frame_names'][0] == 'frame_00000' and (d['frame_clip'] == 1).all()
    assert np.abs(d['transl'] - den[1, :, 16:19]).max() < 1e-6
