"""GPU: rohm_amd.preprocessing_amass -- the `rohm_amass_preprocess` launch against the float64 oracle body model and against
`rohm_smplx_joints`, chunking, and the command line on a small raw tree (preprocessing_amass.py)."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import geometry as G
from oracle.make_golden import frames_inputs
from rohm_amd.utils import synth

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ('root_orient', 'trans', 'pose_body', 'pose_hand', 'pose_jaw', 'pose_eye')


def _layer(seed=0):
    from rohm_amd.body_model import SMPLXLayer
    return SMPLXLayer.from_tensors(synth.synthetic_smplx_tensors(seed)).to(DEV)


def _inputs(seed, N):
    """float64 arrays of N frames (+ N betas rows to pick recordings' shapes from): the float32 inputs of the frames tests widened
    and moved off the float32 grid, so that the cast does something."""
    p, _ = frames_inputs(seed, N)
    g = np.random.Generator(np.random.PCG64(7000 + seed))
    wide = lambda x: x.astype(np.float64) + 1e-9 * g.standard_normal(x.shape)
    a = {'root_orient': wide(p['global_orient']), 'trans': wide(p['transl']), 'pose_body': wide(p['body_pose']),
         'pose_hand': 0.3 * g.standard_normal((N, 90)), 'pose_jaw': 0.3 * g.standard_normal((N, 3)),
         'pose_eye': 0.3 * g.standard_normal((N, 6))}
    return a, wide(p['betas'])


def _rec_of_frame(lengths):
    return np.concatenate([np.full(n, i, np.int32) for i, n in enumerate(lengths)])


def _run(layer, a, betas, rec):
    from rohm_amd.preprocessing_amass import preprocess_frames
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    joints, params = preprocess_frames(layer, {k: dev(a[k]) for k in KEYS}, dev(betas), rec)
    assert joints.dtype == torch.float32 and params.dtype == torch.float32 and joints.is_cuda and params.is_cuda
    return joints.cpu().numpy(), params.cpu().numpy()


def _expected_params(a, betas, rec):
    return np.concatenate([a['root_orient'], a['trans'], betas[rec], a['pose_body'], a['pose_hand'], a['pose_jaw'],
                           a['pose_eye'][:, 0:3], a['pose_eye'][:, 0:3]], axis=1).astype(np.float32)


_ORACLE = {}


def _oracle_joints(a, betas, rec, seed=0):
    """joints[:, :25] of the float64 oracle body model on the float32-cast inputs (all of them, hands and face included)."""
    if seed not in _ORACLE:
        _ORACLE[seed] = G.BodyModel(synth.synthetic_smplx_tensors(seed), dtype=torch.float64)
    t = lambda x: torch.from_numpy(x.astype(np.float32).astype(np.float64))
    out = _ORACLE[seed](betas=t(betas[rec]), global_orient=t(a['root_orient']), body_pose=t(a['pose_body']), transl=t(a['trans']),
                        jaw_pose=t(a['pose_jaw']), leye_pose=t(a['pose_eye'][:, 0:3]), reye_pose=t(a['pose_eye'][:, 0:3]),
                        left_hand_pose=t(a['pose_hand'][:, :45]), right_hand_pose=t(a['pose_hand'][:, 45:]), return_verts=False)
    return out.joints[:, :25].numpy()


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.fixture(scope='module')
def launch():
    """One launch over recordings of 1, 63, 64, 65 and 257 frames with five different betas."""
    lengths = [1, 63, 64, 65, 257]
    N = sum(lengths)
    a, b = _inputs(11, N)
    betas, rec = b[:5], _rec_of_frame(lengths)
    layer = _layer(0)
    joints, params = _run(layer, a, betas, rec)
    return dict(a=a, betas=betas, rec=rec, layer=layer, joints=joints, params=params, N=N)


def test_joints_vs_float64_oracle_and_params_bit_equal(launch):
    L = launch
    assert L['joints'].shape == (L['N'], 25, 3) and L['params'].shape == (L['N'], 178)
    ref = _oracle_joints(L['a'], L['betas'], L['rec'])
    err = np.abs(L['joints'].astype(np.float64) - ref).max(axis=(0, 2))
    print('max |joint error| per joint [m]:', err)
    assert err.max() < 1e-5
    assert np.array_equal(bits(L['params']), bits(_expected_params(L['a'], L['betas'], L['rec'])))


@pytest.mark.parametrize('N', [127, 128, 129, 256])
def test_frame_counts_around_the_workgroup_size(N):
    """A workgroup takes 128 frames, eight elements per lane at a time: one short of it, exactly one, one over, exactly two."""
    a, b = _inputs(17, N)
    rec = _rec_of_frame([N - 100, 100])
    joints, params = _run(_layer(0), a, b[:2], rec)
    assert np.array_equal(bits(params), bits(_expected_params(a, b[:2], rec)))
    assert np.abs(joints.astype(np.float64) - _oracle_joints(a, b[:2], rec)).max() < 1e-5


def test_first_22_joints_are_rohm_smplx_joints_bit_for_bit(launch):
    from rohm_amd.data_loaders.frames import noisy_clip_joints
    p = torch.from_numpy(launch['params'])
    j22 = noisy_clip_joints(launch['layer'], {'global_orient': p[:, 0:3], 'transl': p[:, 3:6], 'betas': p[:, 6:16],
                                              'body_pose': p[:, 16:79]})
    assert np.array_equal(bits(launch['joints'][:, :22]), bits(j22.cpu().numpy()))


def test_hand_jaw_and_eye_inputs_touch_no_joint(launch):
    L = launch
    g = np.random.Generator(np.random.PCG64(12))
    a = dict(L['a'])
    a['pose_hand'], a['pose_jaw'] = g.standard_normal((L['N'], 90)), g.standard_normal((L['N'], 3))
    a['pose_eye'] = g.standard_normal((L['N'], 6))
    joints, params = _run(L['layer'], a, L['betas'], L['rec'])
    assert np.array_equal(bits(joints), bits(L['joints']))
    changed = (bits(params) != bits(L['params'])).any(axis=0)
    assert not changed[:79].any() and changed[79:].all()
    # the right eye is a second copy of the left eye
    assert not np.array_equal(a['pose_eye'][:, 0:3], a['pose_eye'][:, 3:6])
    assert np.array_equal(bits(params[:, 175:178]), bits(params[:, 172:175]))
    assert np.array_equal(bits(params[:, 172:175]), bits(a['pose_eye'][:, 0:3].astype(np.float32)))


def test_edge_rotations_on_the_root_and_on_the_parent_of_the_leaves():
    g = np.random.Generator(np.random.PCG64(13))
    tiny = g.standard_normal((8, 3))
    tiny *= 1e-6 / np.linalg.norm(tiny, axis=1, keepdims=True)
    near_pi = np.concatenate([np.pi * np.eye(3)[i][None] + 1e-4 * g.standard_normal((3, 3)) for i in range(3)])
    edge = np.concatenate([np.zeros((1, 3)), tiny, near_pi])                # 18 rotation vectors
    E = len(edge)
    a, b = _inputs(14, 2 * E)
    a['root_orient'][:E] = edge
    a['pose_body'][E:, 42:45] = edge                                        # joint 15, the parent of joints 22..24
    a['pose_body'][0, :] = 0.0                                              # and one frame with every rotation exactly zero
    a['pose_body'][E, :] = 0.0
    a['root_orient'][E] = 0.0
    rec = np.zeros(2 * E, np.int32)
    joints, _ = _run(_layer(0), a, b[:1], rec)
    assert synth.SMPLX_PARENTS[22:25] == [15, 15, 15]
    err = np.abs(joints.astype(np.float64) - _oracle_joints(a, b[:1], rec)).max(axis=(1, 2))
    print('max |joint error| per frame [m]:', err)
    assert err.max() < 1e-5


def test_betas_move_the_leaf_joints():
    a, b = _inputs(15, 4)
    two = {k: np.concatenate([v[:2], v[:2]]) for k, v in a.items()}         # the same two frames in both recordings
    joints, params = _run(_layer(0), two, b[:2], _rec_of_frame([2, 2]))
    assert np.array_equal(bits(params[:2, 16:]), bits(params[2:, 16:])) and not np.array_equal(params[:2, 6:16], params[2:, 6:16])
    d = np.abs(joints[:2] - joints[2:]).max(axis=(0, 2))
    assert (d[22:25] > 0).all()
    assert np.abs(joints.astype(np.float64) - _oracle_joints(two, b[:2], _rec_of_frame([2, 2]))).max() < 1e-5


def test_a_handle_with_22_joints_is_refused():
    from rohm_amd._lib import RohmHipError
    from rohm_amd.body_model import SMPLXLayer
    t = synth.synthetic_smplx_tensors(0)
    small = SMPLXLayer(t['v_template'], t['shapedirs'], t['J_regressor'][:22], t['parents'][:22]).to(DEV)
    a, b = _inputs(16, 5)
    with pytest.raises(RohmHipError, match='22 joints'):
        _run(small, a, b[:1], np.zeros(5, np.int32))
    torch.cuda.synchronize()
    # the same call with the whole model goes through, and an index outside the betas rows is caught on the host
    _run(_layer(0), a, b[:1], np.zeros(5, np.int32))
    with pytest.raises(ValueError, match='rec_of_frame'):
        _run(_layer(0), a, b[:1], np.array([0, 0, 1, 0, 0], np.int32))
    empty = {k: v[:0] for k, v in a.items()}
    joints, params = _run(_layer(0), empty, b[:1], np.zeros(0, np.int32))
    assert joints.shape == (0, 25, 3) and params.shape == (0, 178)


# ---- trees --------------------------------------------------------------------------------------------------------------------
def _write_raw(path, frames, fps, seed, gender='neutral', model='smplx'):
    a, b = _inputs(seed, max(frames, 3))                           # the generator sets three special rows
    d = {k: v[:frames] for k, v in a.items()}
    betas = np.concatenate([b[0], np.zeros(6)])                             # the files hold 16 shape values; 10 are read
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez(path, mocap_frame_rate=np.array(fps), gender=np.array(gender), surface_model_type=np.array(model), betas=betas, **d)
    return dict(d, betas=betas)


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def _dirs(root):
    return sorted(os.path.relpath(os.path.join(d, x), root) for d, xs, _ in os.walk(root) for x in xs)


def test_chunking_gives_bit_identical_files(tmp_path):
    from rohm_amd.preprocessing_amass import preprocess_dataset
    raw = tmp_path / 'raw'
    for i, n in enumerate([37, 1, 130, 260]):
        _write_raw(str(raw / 'TotalCapture' / 's1' / f'r{i}_stageii.npz'), n, 30.0, 20 + i)
    layer, logs = _layer(0), []
    one = preprocess_dataset(str(raw), 'TotalCapture', str(tmp_path / 'one'), layer, log=logs.append)
    many = preprocess_dataset(str(raw), 'TotalCapture', str(tmp_path / 'many'), layer, chunk_frames=100, log=logs.append)
    assert one['frames'] == many['frames'] == 428 and one['processed'] == many['processed'] and len(one['processed']) == 4
    assert len(one['chunk_seconds']) == 1 and len(many['chunk_seconds']) == 5
    files = _files(str(tmp_path / 'one'))
    assert files == _files(str(tmp_path / 'many')) and len(files) == 8
    for f in files:
        x, y = np.load(str(tmp_path / 'one' / f)), np.load(str(tmp_path / 'many' / f))
        assert x.dtype == y.dtype == np.float32 and x.shape == y.shape and np.array_equal(bits(x), bits(y)), f
    assert np.load(str(tmp_path / 'one' / 'pose_data_fps_30' / 'TotalCapture' / 's1' / 'r3_stageii.npy')).shape == (260, 25, 3)


def _model_dir(base):
    """A model file of the real SMPLX_NEUTRAL.npz layout under <base>/smplx/ (400 shape components, posedirs [V,3,486], ...)."""
    t = synth.synthetic_smplx_tensors(0)
    V = t['v_template'].shape[0]
    sd = np.zeros((V, 3, 400), np.float32)
    sd[:, :, :10], sd[:, :, 300:310] = t['shapedirs'][:, :, :10].numpy(), t['shapedirs'][:, :, 10:].numpy()
    kt = np.stack([np.array(synth.SMPLX_PARENTS), np.arange(55)]).astype(np.int64)
    kt[0, 0] = 2 ** 32 - 1
    os.makedirs(os.path.join(base, 'smplx'))
    np.savez(os.path.join(base, 'smplx', 'SMPLX_NEUTRAL.npz'), v_template=t['v_template'].numpy(), shapedirs=sd,
             posedirs=t['posedirs'].numpy().T.reshape(V, 3, 486), J_regressor=t['J_regressor'].numpy(), kintree_table=kt,
             weights=t['lbs_weights'].numpy(), f=np.zeros((4, 3), np.int64))
    return base


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    """A raw tree of four subsets, and the tool's output for it: ACCAD through `python -m`, the others through main(argv)."""
    from rohm_amd import preprocessing_amass as P
    base = tmp_path_factory.mktemp('amass')
    raw, out, model = str(base / 'raw'), str(base / 'out'), _model_dir(str(base / 'models'))
    src = {}
    w = lambda rel, *args, **kw: src.__setitem__(rel, _write_raw(os.path.join(raw, rel + '.npz'), *args, **kw))
    w('ACCAD/s1/a_stageii', 10, 120.0, 30)
    w('ACCAD/s1/b_stageii', 11, 120.0, 31)
    w('ACCAD/s1/c_100fps_stageii', 10, 100.0, 32)
    w('ACCAD/s1/d_female_stageii', 10, 120.0, 33, gender='female')
    w('ACCAD/s1/e_smplh_stageii', 10, 120.0, 34, model='smplh')
    w('ACCAD/s1/neutral_stagei', 10, 120.0, 35)
    w('ACCAD/s2/neutral_stagei', 10, 120.0, 36)                             # a subject whose only recording is skipped
    w('SSM/s1/slow_stageii', 9, 59.9912, 37)
    w('SSM/s1/fast_stageii', 9, 120.0031, 38)
    w('HDM05/dg/HDM_dg_07-01_01_120_stageii', 8, 120.0, 39)
    w('HDM05/dg/HDM_dg_01-01_01_120_stageii', 8, 120.0, 40)
    w('BMLrub/rub001/0001_treadmill_fast_stageii', 8, 120.0, 41)
    w('BMLrub/rub001/0002_jumping1_stageii', 8, 120.0, 42)
    common = ['--body_model_path', model, '--amass_root', raw, '--save_root', out, '--device', DEV]
    r = subprocess.run([sys.executable, '-m', 'rohm_amd.preprocessing_amass', '--dataset_name', 'ACCAD'] + common, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in ('SSM', 'HDM05', 'BMLrub'):
        assert P.main(['--dataset_name', name] + common) == 0
    return dict(raw=raw, out=out, model=model, src=src, common=common, stdout=r.stdout, base=base)


KEPT = {'ACCAD/s1/a_stageii': (4, 3), 'ACCAD/s1/b_stageii': (4, 3), 'SSM/s1/slow_stageii': (2, 5), 'SSM/s1/fast_stageii': (4, 3),
        'HDM05/dg/HDM_dg_01-01_01_120_stageii': (4, 2), 'BMLrub/rub001/0002_jumping1_stageii': (4, 2)}


def test_command_line_writes_the_scripts_trees(tree):
    out = tree['out']
    assert _files(out) == sorted(f'{t}/{rel}.npy' for t in ('pose_data_fps_30', 'smpl_data_fps_30') for rel in KEPT)
    assert _dirs(out) == sorted(
        [t for t in ('pose_data_fps_30', 'smpl_data_fps_30')] +
        [f'{t}/{d}' for t in ('pose_data_fps_30', 'smpl_data_fps_30')
         for d in ('ACCAD', 'ACCAD/s1', 'ACCAD/s2', 'SSM', 'SSM/s1', 'HDM05', 'HDM05/dg', 'BMLrub', 'BMLrub/rub001')])
    for word in ('gender not neutral', 'not smplx params', 'frame rate 100.0', 'finished.'):
        assert word in tree['stdout'], tree['stdout']
    for rel, (ds, n) in KEPT.items():
        joints, params = np.load(f'{out}/pose_data_fps_30/{rel}.npy'), np.load(f'{out}/smpl_data_fps_30/{rel}.npy')
        assert joints.dtype == np.float32 and joints.shape == (n, 25, 3), rel
        assert params.dtype == np.float32 and params.shape == (n, 178), rel
        s = tree['src'][rel]
        kept = {k: s[k][::ds] for k in KEYS}
        assert len(kept['trans']) == n
        assert np.array_equal(bits(params), bits(_expected_params(kept, s['betas'][None, :10], np.zeros(n, np.int32)))), rel
        assert np.abs(joints.astype(np.float64) - _oracle_joints(kept, s['betas'][None, :10], np.zeros(n, np.int32))).max() < 1e-5, rel


def test_the_loader_reads_the_result(tree):
    from rohm_amd.data_loaders.dataloader_amass import read_amass_clips
    from rohm_amd.data_loaders.frames import noisy_clip_joints
    joints, smplx, starts = read_amass_clips(tree['out'], ['ACCAD'], 'train', clip_len=3)
    assert joints.shape == (6, 22, 3) and smplx.shape == (6, 79) and list(starts) == [0, 3]
    p = torch.from_numpy(smplx.astype(np.float32))
    assert np.array_equal(p.numpy().astype(np.float64), smplx)
    j22 = noisy_clip_joints(_layer(0), {'global_orient': p[:, 0:3], 'transl': p[:, 3:6], 'betas': p[:, 6:16], 'body_pose': p[:, 16:79]})
    assert np.array_equal(bits(joints), bits(j22.cpu().numpy()))


def test_check_against(tree, capsys):
    from rohm_amd import preprocessing_amass as P
    args = ['--dataset_name', 'ACCAD'] + tree['common']
    before = _files(tree['out'])
    assert P.main(args + ['--check_against', tree['out']]) == 0
    text = capsys.readouterr().out
    assert 'max |joints difference| 0.000e+00 m, max |params difference| 0.000e+00' in text and 'different' not in text
    assert _files(tree['out']) == before                                    # nothing is written in this mode

    other = str(tree['base'] / 'perturbed')
    shutil.copytree(tree['out'], other)
    victim = 'pose_data_fps_30/ACCAD/s1/b_stageii.npy'
    np.save(os.path.join(other, victim), np.load(os.path.join(other, victim)) + np.float32(1e-3))
    assert P.main(args + ['--check_against', other]) != 0
    text = capsys.readouterr().out
    assert victim in text and 'a_stageii' not in text
    assert P.main(args + ['--check_against', other, '--check_tol', '2e-3']) == 0
    capsys.readouterr()

    np.save(os.path.join(other, victim), np.load(os.path.join(tree['out'], victim)))
    gone = 'smpl_data_fps_30/ACCAD/s1/a_stageii.npy'
    os.remove(os.path.join(other, gone))
    assert P.main(args + ['--check_against', other]) != 0
    text = capsys.readouterr().out
    assert 'missing' in text and gone in text
    shutil.copy(os.path.join(tree['out'], gone), os.path.join(other, gone))
    shutil.copy(os.path.join(tree['out'], gone), os.path.join(other, 'smpl_data_fps_30/ACCAD/s1/zz_stageii.npy'))
    assert P.main(args + ['--check_against', other]) != 0
    text = capsys.readouterr().out
    assert 'extra' in text and 'zz_stageii.npy' in text
