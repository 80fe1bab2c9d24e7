"""CPU: the host side of rohm_amd.export -- the stitching plan, the repeated-batch rule, the writers and the command line."""
import os
import pickle

import numpy as np
import pytest
import torch

import export_ref as ER
import video_tree as VT
from helpers import golden


def _export():
    from rohm_amd import export
    return export


# ---- plan_frames ---------------------------------------------------------------------------------------------------------
def test_plan_of_the_synthetic_tree():
    """3 clips of T = 7 rows every 6 frames: 19 frames, frames 6 and 12 shared, frame 19 of the 20-frame recording absent."""
    E = _export()
    fc, ft, n = E.plan_frames(3, VT.CLIP_LEN - 1, VT.CLIP_LEN, VT.OVERLAP, keep='first')
    assert n == 19 == len(fc) == len(ft) and fc.dtype == ft.dtype == np.int32
    assert fc.tolist() == [0] * 7 + [1] * 6 + [2] * 6
    assert ft.tolist() == list(range(7)) + list(range(1, 7)) * 2
    lc, lt, n = E.plan_frames(3, 7, 8, 2, keep='last')
    assert n == 19 and lc.tolist() == [0] * 6 + [1] * 6 + [2] * 7 and lt.tolist() == list(range(6)) * 2 + list(range(7))
    # every (clip, row) addresses the recording frame it is exported as; the two plans differ at the shared frames only
    for c, t in ((fc, ft), (lc, lt)):
        assert (c.astype(np.int64) * 6 + t == np.arange(19)).all()
    assert np.flatnonzero(fc != lc).tolist() == [6, 12]


def test_plan_without_shared_frames_and_without_clips():
    E = _export()
    fc, ft, n = E.plan_frames(3, 7, 8, 1)
    assert n == 21 and fc.tolist() == [0] * 7 + [1] * 7 + [2] * 7 and ft.tolist() == list(range(7)) * 3
    assert all(np.array_equal(a, b) for a, b in zip(E.plan_frames(3, 7, 8, 1, 'last')[:2], (fc, ft)))
    fc, ft, n = E.plan_frames(0, 7, 8, 2)
    assert n == 0 and len(fc) == len(ft) == 0 and fc.dtype == np.int32
    assert E.plan_frames(1, 7, 8, 2)[2] == 7
    # the drivers' pose stage keeps clip_len - 2 rows: contiguous clips, nothing shared
    fc, ft, n = E.plan_frames(2, 143, 145, 2)
    assert n == 286 and fc.tolist() == [0] * 143 + [1] * 143
    with pytest.raises(ValueError):
        E.plan_frames(3, 7, 8, 2, keep='both')
    with pytest.raises(ValueError):
        E.plan_frames(3, 7, 8, 8)
    with pytest.raises(ValueError):
        E.plan_frames(3, 4, 8, 2)           # rows every 6 frames, 4 rows each: frames uncovered


# ---- the repeated batch ----------------------------------------------------------------------------------------------------
def test_repeated_first_batch_is_dropped():
    E = _export()
    g = np.random.Generator(np.random.PCG64(3))
    transf = g.standard_normal((8, 4, 4)).astype(np.float32)
    twelve = np.concatenate([transf, transf[:4]])
    assert E.first_pass_rows(twelve) == 8 == ER.repeated_batch_rows(twelve)
    assert E.first_pass_rows(transf) == 8 == ER.repeated_batch_rows(transf)
    assert E.first_pass_rows(transf[:1]) == 1 and E.first_pass_rows(transf[:0]) == 0
    near = twelve.copy()
    near[8, 0, 0] = np.nextafter(near[8, 0, 0], np.float32(np.inf))          # bit for bit, not approximately
    assert E.first_pass_rows(near) == 12
    # the rule is the drivers' schedule: 8 clips in batches of 4 run batches 0, 1, 0
    from rohm_amd.drivers.results import step_schedule
    assert step_schedule(8, 4) == [0, 1, 0] and step_schedule(7, 4) == [0, 1]


# ---- writers ---------------------------------------------------------------------------------------------------------------
def _result(n=5, seed=0):
    E = _export()
    g = np.random.Generator(np.random.PCG64(seed))
    p = torch.from_numpy(g.standard_normal((n, 79)))
    return E.ExportResult(p, torch.from_numpy(g.standard_normal((n, 22, 3)).astype(np.float32)),
                          torch.from_numpy(g.uniform(size=(n, 4)).astype(np.float32)), torch.arange(n, dtype=torch.int32) // 3,
                          torch.arange(n, dtype=torch.int32) % 3, 'camera')


def test_ply_round_trip_is_bit_exact(tmp_path):
    from rohm_amd.occlusion import read_ply
    E = _export()
    g = np.random.Generator(np.random.PCG64(1))
    verts = g.standard_normal((37, 3)).astype(np.float32)
    faces = g.integers(0, 37, size=(50, 3)).astype(np.int32)
    v, f = read_ply(E.write_ply(str(tmp_path / 'm.ply'), verts, faces))
    assert v.dtype == np.float32 and f.dtype == np.int32
    assert v.tobytes() == verts.tobytes() and np.array_equal(f, faces)
    v, f = read_ply(E.write_ply(str(tmp_path / 't.ply'), torch.from_numpy(verts), faces.astype(np.int64)))
    assert v.tobytes() == verts.tobytes() and np.array_equal(f, faces)


def test_obj_writer(tmp_path):
    E = _export()
    verts = np.array([[0, 0, 0], [1, 0, 0.5], [0, 1.25, 0]], np.float32)
    path = E.write_obj(str(tmp_path / 'm.obj'), verts, np.array([[0, 1, 2]]))
    lines = open(path).read().splitlines()
    assert lines[-1] == 'f 1 2 3' and len(lines) == 4
    got = np.array([[float(x) for x in ln.split()[1:]] for ln in lines[:3]], np.float32)
    assert np.array_equal(got, verts)


def test_prox_fits_are_what_the_loader_reads(tmp_path):
    from rohm_amd.data_loaders.dataloader_video import read_fittings
    E = _export()
    res = _result(5)
    names = [f's001_frame_{i + 1:05d}' for i in range(5)]
    d = E.write_prox_fits(str(tmp_path), 'N0Sofa_00034_01', res, names)
    assert d == str(tmp_path / 'N0Sofa_00034_01' / 'results') and sorted(os.listdir(d)) == names
    got = read_fittings(d, names)
    p32 = res.params79.numpy().astype(np.float32)
    for k, (a, b) in E.PARAM_COLS.items():
        assert got[k].dtype == np.float32 and np.array_equal(got[k], p32[:, a:b]), k
    with open(os.path.join(d, names[2], '000.pkl'), 'rb') as f:
        row = pickle.load(f)
    assert {k: v.shape for k, v in row.items()} == {'transl': (1, 3), 'global_orient': (1, 3), 'betas': (1, 10), 'body_pose': (1, 63),
                                                    'jaw_pose': (1, 3), 'leye_pose': (1, 3), 'reye_pose': (1, 3), 'expression': (1, 10)}
    assert all(v.dtype == np.float32 for v in row.values()) and not row['expression'].any() and not row['jaw_pose'].any()
    d = E.write_prox_fits(str(tmp_path / 'ego'), 'rec', res, names, body_idx=1)
    assert d == str(tmp_path / 'ego' / 'rec' / 'body_idx_1' / 'results') and len(os.listdir(d)) == 5
    with pytest.raises(ValueError):
        E.write_prox_fits(str(tmp_path / 'short'), 'rec', res, names[:3])


def test_npz_keys_and_dtypes(tmp_path):
    E = _export()
    res = _result(5)
    names = [f'frame_{i:05d}' for i in range(5)]
    d = np.load(E.write_npz(str(tmp_path / 'rec' / 'smplx_params.npz'), res, names))
    want = {'global_orient': (np.float32, (5, 3)), 'transl': (np.float32, (5, 3)), 'betas': (np.float32, (5, 10)),
            'body_pose': (np.float32, (5, 63)), 'joints': (np.float32, (5, 22, 3)), 'foot_contact': (np.float32, (5, 4)),
            'frame_clip': (np.int32, (5,))}
    assert set(d.files) == set(want) | {'frame_names', 'coordinate_frame', 'gender'}
    for k, (dt, shape) in want.items():
        assert d[k].dtype == dt and d[k].shape == shape, k
    assert d['frame_names'].tolist() == names and str(d['coordinate_frame']) == 'camera' and str(d['gender']) == 'neutral'
    assert np.array_equal(d['body_pose'], res.params79.numpy()[:, 16:79].astype(np.float32))
    assert np.array_equal(d['frame_clip'], [0, 0, 0, 1, 1])


# ---- the command line --------------------------------------------------------------------------------------------------------
def test_cli_arguments():
    E = _export()
    a = E.parse_args(['--dataset', 'egobody', '--saved_data_dir', 'res', '--recordings', 'r1,r2', '--dataset_root', '/data/egobody',
                      '--body_model_path', 'bm', '--out', 'o', '--frame', 'camera', '--formats', 'npz,prox_fits', '--meshes', 'ply',
                      '--mesh_interval', '10', '--keep', 'last', '--betas', 'mean', '--overlap_len', '3', '--init_root', 'init'])
    assert (a.dataset, a.saved_data_dir, a.recordings, a.dataset_root, a.body_model_path, a.out, a.frame) == \
        ('egobody', 'res', ['r1', 'r2'], '/data/egobody', 'bm', 'o', 'camera')
    assert (a.formats, a.meshes, a.mesh_interval, a.keep, a.betas, a.overlap_len, a.init_root) == \
        (['npz', 'prox_fits'], 'ply', 10, 'last', 'mean', 3, 'init')
    d = E.parse_args(['--saved_data_path', 'x.pkl'])
    assert (d.dataset, d.frame, d.formats, d.meshes, d.mesh_interval, d.keep, d.betas, d.overlap_len, d.recordings) == \
        ('prox', 'scene', ['npz'], 'none', 1, 'first', 'frame', 2, [])
    assert E.parse_args(['--dataset', 'amass', '--saved_data_path', 'x.pkl']).dataset == 'amass'
    for bad in (['--saved_data_path', 'x.pkl', '--no_such_argument', '1'], ['--saved_data_path', 'x.pkl', '--formats', 'npz,fbx'],
                ['--saved_data_path', 'x.pkl', '--frame', 'world'], ['--saved_data_path', 'x.pkl', '--dataset', 'h36m'],
                [], ['--saved_data_path', 'x.pkl', '--saved_data_dir', 'd'],
                ['--saved_data_path', 'x.pkl', '--frame', 'camera'],                       # no calibration to read
                ['--saved_data_path', 'x.pkl', '--dataset', 'amass', '--frame', 'camera', '--dataset_root', 'r']):
        with pytest.raises(SystemExit):
            E.parse_args(bad)


def test_export_params_argument_errors():
    E = _export()
    x = np.zeros((3, 7, 294), np.float32)
    with pytest.raises(ValueError):
        E.export_params(x, None, None, frame='world')
    with pytest.raises(ValueError):
        E.export_params(x, None, None, betas='median')
    with pytest.raises(ValueError):
        E.export_params(x, None, None, frame='camera')          # no cam2world


def test_read_cam2world_is_the_loaders(tmp_path):
    """`read_cam2world` was factored out of the EgoBody reader: both readers still return the trees' transforms."""
    from rohm_amd.data_loaders import dataloader_video as DV
    g = golden('video_loader.npz')
    for dataset in ('prox', 'egobody'):
        a = VT.tree_arrays_from_fixture(g, dataset)
        paths = VT.write_tree(str(tmp_path / dataset), dataset, a)
        rec = str(a['recording_name'])
        want = a['cam2world'] if dataset == 'prox' else a['master2world'] @ a['sub2main']
        got = DV.read_cam2world(dataset, paths['base_dir'], rec)
        assert got.dtype == np.float64 and np.array_equal(got, want)
        read = DV.read_prox_recording if dataset == 'prox' else DV.read_egobody_recording
        full = read(paths['init_root'], paths['base_dir'], rec)
        assert np.array_equal(full['cam2world'], want)
        if dataset == 'egobody':
            assert np.array_equal(full['master2world'], a['master2world'])
    with pytest.raises(ValueError):
        DV.read_cam2world('amass', str(tmp_path), 'x')
