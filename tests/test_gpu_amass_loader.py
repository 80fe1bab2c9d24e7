"""GPU: the native DataloaderAMASS (rohm_amd/data_loaders/dataloader_amass.py) on the AMASS tree rebuilt from
tests/golden/amass_loader.npz, against everything the reference's own DataloaderAMASS produced on that tree
(scripts/make_golden_amass.py): cases a (train, task 'pose', drawn noise), b (test, spacing 2, loaded noise, task 'traj' with
repr_abs_only), c (no input noise) and d (sep_noise).

Bars.  Clean geometry and the noisy joints of the device's forward kinematics: 5e-6 (GEOM_TOL of tests/test_gpu_clips.py).
Noisy parameters from the fixture's noise: 1e-9 (float64; orders above the rounding of angles up to 180 degrees, two below the
float32 cast that follows).  Representations of fixture inputs: the `_close` rule of tests/test_gpu_clips.py.  End to end the
noisy representation is made of the DEVICE's joints, which may differ from the fixture's by 5e-6; the `_close` limits are
widened per REPR_LIST group by 4x the largest change that uniform +-5e-6 perturbations of the fixture's noisy joints cause
in the restatement (8 draws, cases a and b; tests/amass_ref.py::JOINT_WIDENING, re-measured on the CPU by
tests/test_amass_ref.py::test_joint_widening_measurement), in de-normalised units:
    root_rot_angle 8.166e-05, root_rot_angle_vel 1.070e-04, root_l_pos 5.000e-06, root_l_vel 1.405e-05, root_height 4.992e-06,
    local_positions 4.397e-05, local_vel 2.133e-05, the parameter-only groups 0.
Contact channels are compared exactly, except decisions within a relative 1e-2 of a threshold, which must stay <= 1 % of the
decisions (none in this fixture).  Normalised items are compared after de-normalising with the reference's Mean / Std at the
same bars.  Mean / Std: 4x the distance of the reference's float32-accumulated values from a float64 computation on its
own arrays, as stored in the fixture (4.9e-7 and 1.5e-8)."""
import pickle

import numpy as np
import pytest
import torch

import amass_ref as AR
import clips_ref as CR
from helpers import golden
from oracle import geometry as G
from rohm_amd.utils import synth

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GEOM_TOL = 5e-6
PARAM_TOL = 1e-9
LOCAL_FACTOR = 4 * 0.0112
DATASETS = list(AR.TREE)


def _layer():
    from rohm_amd.body_model import SMPLXLayer
    return SMPLXLayer.from_tensors(synth.synthetic_smplx_tensors(0)).to(DEV)


@pytest.fixture(scope='module')
def fx(tmp_path_factory):
    g = golden('amass_loader.npz')
    root = AR.write_tree(str(tmp_path_factory.mktemp('amass')), AR.fixture_tree(g))
    logdir = str(tmp_path_factory.mktemp('log'))
    for name, key in (('AMASS_mean.pkl', 'mean_pkl'), ('AMASS_std.pkl', 'std_pkl')):        # the reference's own pickles
        with open(f'{logdir}/{name}', 'wb') as f:
            f.write(g[key].tobytes())
    return g, root, logdir


def _loader(fx, logdir=None, **kw):
    from rohm_amd.data_loaders.dataloader_amass import DataloaderAMASS
    g, root, ref_logdir = fx
    return DataloaderAMASS(preprocessed_amass_root=root, body_model_path=_layer(), amass_datasets=DATASETS,
                           clip_len=int(g['clip_len']), logdir=logdir or ref_logdir, device=DEV, **kw)


@pytest.fixture(scope='module')
def case_a(fx, tmp_path_factory):
    np.random.seed(int(fx[0]['seed_a']))
    logdir = str(tmp_path_factory.mktemp('log_a'))
    return _loader(fx, logdir, split='train', task='pose', input_noise=True, **AR.STAGE1_STD), logdir


@pytest.fixture(scope='module')
def case_b(fx):
    noise = {k: fx[0]['b_noise_' + k] for k in AR.NOISE_ORDER}
    return _loader(fx, split='test', spacing=2, task='traj', repr_abs_only=True, input_noise=True, load_noise=True,
                   loaded_smplx_noise_dict=noise, **AR.STAGE2_STD)


def _close(out, ref, joints, widening=None, allow_near=False):
    """tests/test_gpu_clips.py::_close, optionally widened (module docstring)."""
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    lim = AR.widened_limits(ref, joints, widening or {}, 2e-5, LOCAL_FACTOR)
    err = np.abs(out - ref)
    print(f'max err {err[..., :290].max():.3e} (largest limit {lim.max():.3e}, smallest {lim.min():.3e})')
    assert (err[..., :290] <= lim[..., :290]).all(), f'outside tolerance at {np.argwhere(err > lim)[:5].tolist()}'
    near = AR.near_threshold(joints) if allow_near else np.zeros(out[..., 290:].shape, bool)
    assert near.mean() <= 0.01
    assert np.array_equal(out[..., 290:][~near], ref[..., 290:][~near])


def _device_lists(ds):
    return {k: v.cpu().numpy() for k, v in ds._device_data.items()}


def test_clean_side_against_the_reference(fx):
    """Canonical joints, float32 and float64 parameters, transf and the clean representation of the train clips."""
    from rohm_amd.data_loaders import clips
    from rohm_amd.data_loaders.dataloader_amass import read_amass_clips
    g, root, _ = fx
    joints, smplx, starts = read_amass_clips(root, DATASETS, 'train', 16)
    assert joints.shape == (64, 22, 3) and joints.dtype == np.float32 and smplx.shape == (64, 79) and smplx.dtype == np.float64
    assert starts.tolist() == [0, 16, 32, 48] and starts.dtype == np.int32
    assert read_amass_clips(root, DATASETS, 'test', 16)[2].tolist() == [0, 16, 32]
    J, W = torch.from_numpy(joints).to(DEV), torch.from_numpy(smplx).to(DEV)
    st = torch.from_numpy(starts).to(DEV)
    out = clips.build_clips(J, W, 16, 0, starts=st, params_f64=True)
    plain = clips.build_clips(J, W, 16, 0, starts=st)
    for k in plain:                                         # the float64 output changes nothing else
        assert torch.equal(out[k], plain[k]), k
    assert np.abs(out['cano_joints'].cpu().numpy() - g['a_joints_clean']).max() <= GEOM_TOL
    assert np.abs(out['transf_matrix'].cpu().numpy() - g['a_transf']).max() <= GEOM_TOL
    ot = out['orient_transl64'].cpu().numpy()
    assert ot.dtype == np.float64 and ot.shape == (4, 16, 6)
    for k, cols in (('global_orient', slice(0, 3)), ('transl', slice(3, 6))):
        assert np.abs(out[k].cpu().numpy() - g['a_params_' + k]).max() <= GEOM_TOL, k
        assert np.abs(ot[..., cols] - g['a_params_' + k]).max() <= PARAM_TOL, k
        assert np.array_equal(ot[..., cols].astype(np.float32), out[k].cpu().numpy()), k
    _close(out['repr'].cpu().numpy(), g['a_repr_clean'], g['a_joints_clean'])
    # a window that leaves the frames: NaN in the float64 output too
    off = clips.build_clips(J, W, 16, 0, starts=torch.tensor([60], device=DEV, dtype=torch.int32), params_f64=True)
    assert torch.isnan(off['orient_transl64']).all() and torch.isnan(off['repr']).all()


@pytest.mark.parametrize('case,n', [('a_', 4), ('b_', 2)])
def test_noise_kernel_and_fk_on_the_fixture_noise(fx, case, n):
    """Noisy parameters (float64, from the fixture's canonical parameters and noise), then the noisy joints."""
    from rohm_amd.data_loaders import frames
    from rohm_amd.data_loaders.dataloader_amass import PARAM_COLS, param_noise
    g = fx[0]
    rows = np.stack([AR.rows79(p) for p in AR.fixture_params(g, case + 'params_', n)])
    pick = [0, 4] if case == 'b_' else list(range(n))
    noise = {k: torch.from_numpy(np.ascontiguousarray(g[case + 'noise_' + k][pick])).to(DEV) for k in AR.NOISE_ORDER}
    out = param_noise(torch.from_numpy(rows).to(DEV), noise)
    want = np.stack([AR.rows79(p) for p in AR.fixture_params(g, case + 'noisy_', n)])
    err = np.abs(out.cpu().numpy() - want).max()
    print(f'noisy parameters: max err {err:.3e}')
    assert err <= PARAM_TOL
    flat = out.reshape(n * 16, 79)
    fk = frames.noisy_clip_joints(_layer(), {k: flat[:, a:b] for k, (a, b) in PARAM_COLS.items()}, DEV).reshape(n, 16, 22, 3)
    err = np.abs(fk.cpu().numpy() - g[case + 'joints_noisy']).max()
    print(f'noisy joints: max err {err:.3e}')
    assert fk.dtype == torch.float32 and err <= GEOM_TOL


@pytest.mark.parametrize('case,n', [('a_', 4), ('b_', 2)])
def test_clips_repr_on_the_fixture_noisy_clips(fx, case, n):
    from rohm_amd.data_loaders.clips import clips_repr
    g = fx[0]
    rows = np.stack([AR.rows79(p) for p in AR.fixture_params(g, case + 'noisy_', n)])
    joints = g[case + 'joints_noisy']
    assert joints.dtype == np.float32
    out = clips_repr(torch.from_numpy(joints).to(DEV), torch.from_numpy(rows).to(DEV))
    _close(out.cpu().numpy(), g[case + 'repr_noisy'], joints)


def _check_items(ds, g, p, n, keys, noisy_ref=None, joints_ref=None, overwrite=0):
    """Host items against the reference's, de-normalised with the reference's Mean / Std."""
    mean, std = g['Mean'].astype(np.float64), g['Std'].astype(np.float64)
    own_mean, own_std = ds.Mean.astype(np.float64), ds.Std.astype(np.float64)
    for i in range(n):
        item = ds[i]
        assert list(item) == keys
        clean_ref = g[f'a_item{i}_motion_repr_clean'] if p in ('c_', 'd_') else g[f'{p}item{i}_motion_repr_clean']
        assert item['motion_repr_clean'].dtype == np.float32 and item['motion_repr_clean'].shape == clean_ref.shape
        cj = g[('b_' if p == 'b_' else 'a_') + 'joints_clean'][i][None]
        _close((item['motion_repr_clean'] * own_std + own_mean)[None], (clean_ref * std + mean)[None], cj)
        if 'noisy_joints' in item:
            ref_j = g[f'{p}item{i}_noisy_joints']
            assert item['noisy_joints'].dtype == ref_j.dtype == np.float32 and item['noisy_joints'].shape == ref_j.shape
            assert np.abs(item['noisy_joints'] - ref_j).max() <= GEOM_TOL
            ref_n = g[f'{p}item{i}_motion_repr_noisy']
            assert item['motion_repr_noisy'].dtype == np.float32 and item['motion_repr_noisy'].shape == ref_n.shape
            wide = {k: (0.0 if AR.GROUPS[k][1] <= overwrite else v) for k, v in AR.JOINT_WIDENING.items()}
            _close((item['motion_repr_noisy'] * own_std + own_mean)[None], (ref_n * std + mean)[None], ref_j[None], wide, True)
        else:
            assert np.array_equal(item['motion_repr_noisy'], item['motion_repr_clean'])
        if 'cond' in item:
            t = item['motion_repr_noisy']
            assert np.array_equal(item['cond'], t[:, AR.ABS_TRAJ_CH] if ds.repr_abs_only else t[:, :22])
            assert np.array_equal(item['control_cond'], item['motion_repr_clean'][:, -272:])
            assert item['cond'].dtype == item['control_cond'].dtype == np.float32


def test_case_a_end_to_end(fx, case_a):
    g = fx[0]
    ds, logdir = case_a
    assert (ds.n_samples, len(ds), ds.clip_len) == (4, 4, 16)
    for attr in ('body_feat_dim', 'traj_feat_dim', 'pose_feat_dim', 'n_samples', 'clip_len'):
        assert getattr(ds, attr) == int(g['a_' + attr]), attr
    # np.random.seed(k) reproduces the reference's draws bit for bit
    for k in AR.NOISE_ORDER:
        assert np.array_equal(ds.smplx_noise_dict[k], g['a_noise_' + k]), k
    d = _device_lists(ds)
    assert np.abs(d['joints_clean'] - g['a_joints_clean']).max() <= GEOM_TOL
    _close(d['clean'], g['a_repr_clean'], g['a_joints_clean'])
    assert np.abs(d['joints_noisy'] - g['a_joints_noisy']).max() <= GEOM_TOL
    _close(d['noisy'], g['a_repr_noisy'], g['a_joints_noisy'], AR.JOINT_WIDENING, True)
    assert set(np.unique(d['noisy'][..., 290:])) == {0.0, 1.0}
    # statistics and their pickles
    dm, dstd = np.abs(ds.Mean - g['Mean']).max(), np.abs(ds.Std - g['Std']).max()
    print(f'Mean err {dm:.3e} (bar {float(g["mean_bar"]):.3e}), Std err {dstd:.3e} (bar {float(g["std_bar"]):.3e})')
    assert dm <= float(g['mean_bar']) and dstd <= float(g['std_bar'])
    assert ds.Mean.dtype == ds.Std.dtype == np.float32 and ds.Mean.shape == ds.Std.shape == (294,)
    ref_mean, ref_std = AR.fixture_stats(g)
    for fname, ref, own in (('AMASS_mean.pkl', ref_mean, ds.Mean_dict), ('AMASS_std.pkl', ref_std, ds.Std_dict)):
        with open(f'{logdir}/{fname}', 'rb') as f:
            got = pickle.load(f)
        assert isinstance(got, dict) and list(got) == list(ref) == G.REPR_LIST
        for k in ref:
            assert got[k].dtype == ref[k].dtype == np.float32 and got[k].shape == ref[k].shape and np.array_equal(got[k], own[k])
    assert (ds.Mean_dict['foot_contact'] == 0).all() and (ds.Std_dict['foot_contact'] == 1).all()
    _check_items(ds, g, 'a_', 4, ['motion_repr_clean', 'noisy_joints', 'motion_repr_noisy'], overwrite=22)
    for i in range(4):                                      # task 'pose': clean trajectory channels, written before normalising
        item = ds[i]
        assert np.array_equal(item['motion_repr_noisy'][:, :22], item['motion_repr_clean'][:, :22])
        assert not np.array_equal(item['motion_repr_noisy'][:, 22:], item['motion_repr_clean'][:, 22:])


def test_case_b_end_to_end(fx, case_b):
    g, ds = fx[0], case_b
    assert (ds.n_samples, len(ds), ds.traj_feat_dim, ds.pose_feat_dim) == (3, 1, 13, 272) == \
        (int(g['b_n_samples']), int(g['b_len']), int(g['b_traj_feat_dim']), int(g['b_pose_feat_dim']))
    assert np.array_equal(ds.Mean, g['Mean']) and np.array_equal(ds.Std, g['Std'])          # read from the pickles
    for k in AR.NOISE_ORDER:                                # rows i * spacing of the loaded noise with i = 0, 2
        assert np.array_equal(ds.smplx_noise_dict[k], g['b_noise_' + k][[0, 4]]), k
    d = _device_lists(ds)
    assert d['clean'].shape == (2, 15, 294)                 # ceil(3 / 2) clips are built, __len__ is 3 // 2
    assert np.abs(d['joints_clean'] - g['b_joints_clean']).max() <= GEOM_TOL
    _close(d['clean'], g['b_repr_clean'], g['b_joints_clean'])
    assert np.abs(d['joints_noisy'] - g['b_joints_noisy']).max() <= GEOM_TOL
    _close(d['noisy'], g['b_repr_noisy'], g['b_joints_noisy'], AR.JOINT_WIDENING, True)
    _check_items(ds, g, 'b_', 2, ['motion_repr_clean', 'noisy_joints', 'motion_repr_noisy', 'cond', 'control_cond'])
    assert ds[0]['cond'].shape == (15, 13) and ds[0]['control_cond'].shape == (15, 272)


def test_case_c_without_input_noise(fx, tmp_path):
    g = fx[0]
    ds = _loader(fx, str(tmp_path), split='train', task='traj')
    assert np.abs(ds.Mean - g['Mean']).max() <= float(g['mean_bar']) and np.abs(ds.Std - g['Std']).max() <= float(g['std_bar'])
    _check_items(ds, g, 'c_', 4, ['motion_repr_clean', 'motion_repr_noisy', 'cond', 'control_cond'])
    assert ds[0]['cond'].shape == (15, 22)
    for b in ds.batches(4):
        assert torch.equal(b['motion_repr_noisy'], b['motion_repr_clean']) and 'noisy_joints' not in b


def test_case_d_sep_noise(fx, tmp_path):
    g = fx[0]
    ds = _loader(fx, str(tmp_path), split='train', task='traj', input_noise=True, sep_noise=True,
                 noise_std_joint=AR.SEP_STD_JOINT, **AR.SEP_STD)
    np.random.seed(int(g['seed_d']))
    _check_items(ds, g, 'd_', 4, ['motion_repr_clean', 'noisy_joints', 'motion_repr_noisy', 'cond', 'control_cond'])
    contact = np.stack([g[f'd_item{i}_motion_repr_noisy'][:, 290:] for i in range(4)])
    assert set(np.unique(contact)) == {0.0, 1.0}
    # batches() draws on the device from the generator: reproducible, and the noise is of the requested size
    gen = lambda: torch.Generator(device=DEV).manual_seed(3)
    one, two = list(ds.batches(3, generator=gen())), list(ds.batches(3, generator=gen()))
    assert [b['cond'].shape[0] for b in one] == [3, 1]
    for x, y in zip(one, two):
        assert all(torch.equal(x[k], y[k]) for k in x)
    clean_j = ds._device_data['joints_clean']
    dj = torch.cat([b['noisy_joints'] for b in one]) - clean_j
    assert 0.5e-4 < float(dj.std()) < 2e-4 and one[0]['noisy_joints'].dtype == torch.float32
    assert not torch.equal(one[0]['motion_repr_noisy'][..., 22:290], one[0]['motion_repr_clean'][..., 22:290])


def test_batches(fx, case_a, case_b):
    ds = case_a[0]
    got = list(ds.batches(3))
    assert [b['motion_repr_clean'].shape[0] for b in got] == [3, 1]          # a partial last batch
    assert [b['motion_repr_clean'].shape[0] for b in ds.batches(3, drop_last=True)] == [3]
    want = {'motion_repr_clean': (15, 294), 'noisy_joints': (16, 22, 3), 'motion_repr_noisy': (15, 294)}
    for b in got:
        assert list(b) == list(want)
        for k, s in want.items():
            assert b[k].is_cuda and b[k].dtype == torch.float32 and tuple(b[k].shape[1:]) == s, k
    rows = {k: torch.cat([b[k] for b in got]).cpu().numpy() for k in want}
    for i in range(4):                                      # batch rows are the __getitem__ rows, bit for bit
        item = ds[i]
        for k in want:
            assert np.array_equal(rows[k][i], item[k]), k
    assert np.array_equal(rows['motion_repr_noisy'][..., :22], rows['motion_repr_clean'][..., :22])      # task 'pose'
    # shuffle: a permutation of the unshuffled rows, reproducible from the generator
    for gen in (lambda: torch.Generator().manual_seed(7), lambda: torch.Generator(device=DEV).manual_seed(7)):
        sh = {k: torch.cat([b[k] for b in ds.batches(3, shuffle=True, generator=gen())]).cpu().numpy() for k in want}
        perm = [int(np.flatnonzero([(sh['motion_repr_clean'][j] == rows['motion_repr_clean'][i]).all() for i in range(4)])[0])
                for j in range(4)]
        assert sorted(perm) == [0, 1, 2, 3]
        for k in want:
            assert np.array_equal(sh[k], rows[k][perm]), k
        again = torch.cat([b['motion_repr_clean'] for b in ds.batches(3, shuffle=True, generator=gen())]).cpu().numpy()
        assert np.array_equal(again, sh['motion_repr_clean'])
    # the host items collate to the same batches without the GPU; a worker's copy carries no device state
    for b, hb in zip(got, torch.utils.data.DataLoader(ds, batch_size=3, shuffle=False)):
        for k in want:
            assert torch.equal(b[k].cpu(), hb[k]), k
    clone = pickle.loads(pickle.dumps(ds))
    assert not hasattr(clone, '_device_data') and not hasattr(clone, 'smplx_neutral')
    assert np.array_equal(clone[2]['motion_repr_noisy'], ds[2]['motion_repr_noisy'])
    # task 'traj' with repr_abs_only, spacing 2: __len__ = 1 item although two clips were built
    tb = list(case_b.batches(4))
    assert len(tb) == 1 and list(tb[0]) == ['motion_repr_clean', 'noisy_joints', 'motion_repr_noisy', 'cond', 'control_cond']
    b = tb[0]
    assert tuple(b['cond'].shape) == (1, 15, 13) and tuple(b['control_cond'].shape) == (1, 15, 272)
    assert torch.equal(b['cond'], b['motion_repr_noisy'][..., AR.ABS_TRAJ_CH])
    assert torch.equal(b['control_cond'], b['motion_repr_clean'][..., -272:])
    item = case_b[0]
    for k in b:
        assert np.array_equal(b[k][0].cpu().numpy(), item[k]), k


def test_traj_cond_22_channels_and_spacing_lengths(fx):
    np.random.seed(1)
    ds = _loader(fx, split='test', spacing=2, task='traj', input_noise=True, **AR.STAGE1_STD)
    assert (ds.n_samples, len(ds), ds.traj_feat_dim) == (3, 1, 22) and ds._device_data['clean'].shape[0] == 2
    assert ds.smplx_noise_dict['body_pose'].shape == (2, 16, 21, 3)
    b = next(iter(ds.batches(2)))
    assert tuple(b['cond'].shape) == (1, 15, 22) and torch.equal(b['cond'], b['motion_repr_noisy'][..., :22])
    assert not torch.equal(b['motion_repr_noisy'][..., :22], b['motion_repr_clean'][..., :22])
    assert ds[1]['cond'].shape == (15, 22)                  # the second built clip is there, as in the reference
    ds3 = _loader(fx, split='test', spacing=3, task='pose')
    assert (ds3.n_samples, len(ds3)) == (3, 1) and ds3._device_data['clean'].shape[0] == 1


def test_loader_errors(fx):
    from rohm_amd._lib import RohmHipError
    from rohm_amd.data_loaders.dataloader_amass import DataloaderAMASS
    g, root, logdir = fx
    kw = dict(preprocessed_amass_root=root, body_model_path=_layer(), amass_datasets=DATASETS, clip_len=16, logdir=logdir,
              split='test')
    with pytest.raises(RohmHipError):
        DataloaderAMASS(device='cpu', **kw)
    for bad in (dict(task='both'), dict(split='val'), dict(spacing=0), dict(clip_len=1), dict(joints_num=25),
                dict(input_noise=True, load_noise=True), dict(chunk_clips=0)):
        with pytest.raises(ValueError):
            DataloaderAMASS(device=DEV, **dict(kw, **bad))
    assert len(DataloaderAMASS(device=DEV, **dict(kw, clip_len=64))) == 0                  # no sequence is that long
    with pytest.raises(ValueError):
        next(DataloaderAMASS(device=DEV, **kw).batches(0))
    # chunks of one clip give the same dataset as one chunk
    np.random.seed(5)
    one = DataloaderAMASS(device=DEV, input_noise=True, chunk_clips=1, **dict(kw, **AR.STAGE1_STD))
    np.random.seed(5)
    all_ = DataloaderAMASS(device=DEV, input_noise=True, **dict(kw, **AR.STAGE1_STD))
    for k in ('clean', 'noisy', 'joints_noisy'):
        assert torch.equal(one._device_data[k], all_._device_data[k]), k
