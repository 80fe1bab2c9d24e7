"""CPU: the numpy / scipy restatement of the AMASS loader (tests/amass_ref.py) against the reference's own loader
(tests/golden/amass_loader.npz, scripts/make_golden_amass.py), the properties of the fixture that the GPU tests rely on,
and the measurement behind the widened bars of tests/test_gpu_amass_loader.py."""
import pickle

import numpy as np
import pytest

import amass_ref as AR
import clips_ref as CR
from helpers import golden
from oracle import geometry as G
from rohm_amd.utils import synth

F64_TOL = 1e-12          # float64 quantities restated with the same numpy / scipy calls: rounding-order differences only


@pytest.fixture(scope='module')
def fx(tmp_path_factory):
    g = golden('amass_loader.npz')
    root = AR.write_tree(str(tmp_path_factory.mktemp('amass')), AR.fixture_tree(g))
    body = G.BodyModel(synth.synthetic_smplx_tensors(0))
    return g, root, body


def _loader(fx, **kw):
    g, root, body = fx
    return AR.Loader(root, body, list(AR.TREE), clip_len=int(g['clip_len']), **kw)


def _stack(dicts, k, shape):
    return np.asarray([d[k] for d in dicts]).reshape(shape)


def test_fixture_tree_is_the_synthetic_tree():
    g = golden('amass_loader.npz')
    tree, want = AR.fixture_tree(g), AR.tree_arrays()
    assert sorted(tree) == sorted(want) and int(g['clip_len']) == AR.CLIP_LEN
    for k in want:
        assert np.array_equal(tree[k][0], want[k][0]) and np.array_equal(tree[k][1], want[k][1])
        assert tree[k][0].dtype == np.float32 and tree[k][1].dtype == np.float64
    assert (int(g['seed_a']), int(g['seed_b']), int(g['seed_d'])) == (AR.SEED_A, AR.SEED_B, AR.SEED_D)


def test_fixture_properties():
    """What scripts/make_golden_amass.py asserted on the reference's own output, asserted again."""
    g = golden('amass_loader.npz')
    for p, n in (('a_', 4), ('b_', 2)):
        clean, noisy = g[p + 'repr_clean'], g[p + 'repr_noisy']
        assert clean.shape == noisy.shape == (n, 15, 294) and not np.isnan(clean).any() and not np.isnan(noisy).any()
        assert set(np.unique(clean[..., 290:])) == {0.0, 1.0}
        assert AR.near_threshold(g[p + 'joints_noisy']).mean() <= 0.01
        mid, ang = AR.euler_margins(AR.fixture_params(g, p + 'params_', n), AR.fixture_params(g, p + 'noisy_', n))
        assert mid > 5.0 and ang > 1e-3
    assert set(np.unique(g['a_repr_noisy'][..., 290:])) == {0.0, 1.0}
    d_contact = np.stack([g[f'd_item{i}_motion_repr_noisy'][:, 290:] for i in range(4)])
    assert set(np.unique(d_contact)) == {0.0, 1.0}
    assert AR.near_threshold(np.stack([g[f'd_item{i}_noisy_joints'] for i in range(4)])).mean() <= 0.01
    assert g['b_noise_transl'].shape == (5, 16, 3) and g['b_noise_body_pose'].shape == (5, 16, 21, 3)
    assert (int(g['b_n_samples']), int(g['b_len']), int(g['b_traj_feat_dim'])) == (3, 1, 13)
    assert (int(g['a_n_samples']), int(g['a_traj_feat_dim']), int(g['a_pose_feat_dim']), int(g['a_body_feat_dim'])) == (4, 22, 272, 294)
    assert 0 < float(g['mean_bar']) < 1e-6 and 0 < float(g['std_bar']) < 1e-7


def test_euler_formulas_match_scipy():
    from scipy.spatial.transform import Rotation as R
    g = np.random.Generator(np.random.PCG64(0))
    v = g.standard_normal((500, 3))
    v *= g.uniform(0, 3.1, (500, 1)) / np.linalg.norm(v, axis=1, keepdims=True)
    e = R.from_rotvec(v).as_euler('zxy', degrees=True)
    ok = np.abs(e[:, 1]) < 85
    assert ok.sum() > 400 and np.abs(AR.euler_zxy(v) - e)[ok].max() < 1e-11
    assert np.abs(AR.perturb_rotvec(v[ok], 0.0) - v[ok]).max() < 1e-12


def _check_lists(ds, g, p, n):
    L = int(g['clip_len'])
    assert np.abs(np.asarray(ds.joints_clean) - g[p + 'joints_clean']).max() <= F64_TOL
    for k in AR.PARAM_NAMES:
        assert np.abs(_stack(ds.params, k, g[p + 'params_' + k].shape) - g[p + 'params_' + k]).max() <= F64_TOL, k
        assert np.abs(_stack(ds.params_noisy, k, g[p + 'noisy_' + k].shape) - g[p + 'noisy_' + k]).max() <= F64_TOL, k
    # float32 joints of the same body model from parameters that agree to 1e-12: an ulp of a coordinate at most
    assert np.abs(np.asarray(ds.joints_noisy) - g[p + 'joints_noisy']).max() <= 2.4e-7
    assert np.abs(ds.repr_clean - g[p + 'repr_clean']).max() <= F64_TOL
    assert np.array_equal(ds.repr_clean[..., 290:], g[p + 'repr_clean'][..., 290:])
    lim = CR.repr_limits(g[p + 'repr_noisy'], g[p + 'joints_noisy'].astype(np.float64), None, 1e-6, 4 * 0.0112)
    assert (np.abs(np.asarray(ds.repr_noisy) - g[p + 'repr_noisy']) <= lim).all()
    assert np.array_equal(np.asarray(ds.repr_noisy)[..., 290:], g[p + 'repr_noisy'][..., 290:])
    assert len(ds.joints_clean) == n and ds.repr_clean.shape == (n, L - 1, 294)


def _check_items(ds, g, p, n, keys):
    mean, std = g['Mean'].astype(np.float64), g['Std'].astype(np.float64)
    for i in range(n):
        item = ds[i]
        assert list(item) == keys
        for k in ('motion_repr_clean', 'motion_repr_noisy'):
            name = f'{p}item{i}_{k}'
            if name in g.files:
                assert item[k].dtype == np.float32 and item[k].shape == g[name].shape
                back, ref = item[k] * ds.Std.astype(np.float64) + ds.Mean, g[name] * std + mean
                assert np.abs(back - ref).max() <= 2e-6, k          # float32 rounding of normalised values up to 1 / Std
        if 'noisy_joints' in item:
            assert item['noisy_joints'].dtype == np.float32
            assert np.abs(item['noisy_joints'] - g[f'{p}item{i}_noisy_joints']).max() <= 2.4e-7


def test_case_a_train_pose_drawn_noise(fx):
    g = fx[0]
    np.random.seed(int(g['seed_a']))
    ds = _loader(fx, split='train', task='pose', input_noise=True, **AR.STAGE1_STD)
    for k in AR.NOISE_ORDER:
        assert np.array_equal(np.asarray([n[k] for n in ds.noise]), g['a_noise_' + k]), k
    _check_lists(ds, g, 'a_', 4)
    assert np.abs(np.asarray(ds.transf) - g['a_transf']).max() <= F64_TOL
    assert len(ds) == 4 and ds.n_samples == 4
    assert np.abs(ds.Mean - g['Mean']).max() <= float(g['mean_bar']) and np.abs(ds.Std - g['Std']).max() <= float(g['std_bar'])
    ref_mean, ref_std = AR.fixture_stats(g)
    assert list(ref_mean) == list(ds.Mean_dict) == G.REPR_LIST and list(ref_std) == list(ds.Std_dict)
    for k in ref_mean:
        assert ref_mean[k].dtype == ref_std[k].dtype == np.float32 and ref_mean[k].shape == ds.Mean_dict[k].shape == (G.REPR_DIM[k],)
    _check_items(ds, g, 'a_', 4, ['motion_repr_clean', 'noisy_joints', 'motion_repr_noisy'])
    # task 'pose': the trajectory channels of the noisy item are the clean ones
    for i in range(4):
        assert np.array_equal(g[f'a_item{i}_motion_repr_noisy'][:, :22], g[f'a_item{i}_motion_repr_clean'][:, :22])
        assert not np.array_equal(g[f'a_item{i}_motion_repr_noisy'][:, 22:], g[f'a_item{i}_motion_repr_clean'][:, 22:])


def test_case_b_test_split_spacing_loaded_noise(fx):
    g = fx[0]
    noise = {k: g['b_noise_' + k] for k in AR.NOISE_ORDER}
    ds = _loader(fx, split='test', spacing=2, task='traj', repr_abs_only=True, input_noise=True, load_noise=True,
                 loaded_smplx_noise_dict=noise, stats=AR.fixture_stats(g), **AR.STAGE2_STD)
    assert ds.n_samples == 3 and len(ds) == 1 and len(ds.joints_clean) == 2
    for k in AR.NOISE_ORDER:                                # rows i * spacing with i = 0, 2: the reference's quirk
        assert np.array_equal(np.asarray([n[k] for n in ds.noise]), noise[k][[0, 4]]), k
    _check_lists(ds, g, 'b_', 2)
    assert np.array_equal(ds.Mean, g['Mean']) and np.array_equal(ds.Std, g['Std'])
    _check_items(ds, g, 'b_', 2, ['motion_repr_clean', 'noisy_joints', 'motion_repr_noisy', 'cond', 'control_cond'])
    assert ds[0]['cond'].shape == (15, 13) and ds[0]['control_cond'].shape == (15, 272)


def test_case_c_without_input_noise(fx):
    g = fx[0]
    ds = _loader(fx, split='train', task='traj')
    assert np.abs(ds.repr_clean - g['a_repr_clean']).max() <= F64_TOL
    mean, std = g['Mean'].astype(np.float64), g['Std'].astype(np.float64)
    for i in range(4):
        item = ds[i]
        assert list(item) == ['motion_repr_clean', 'motion_repr_noisy', 'cond', 'control_cond']
        assert np.array_equal(item['motion_repr_noisy'], item['motion_repr_clean']) and item['cond'].shape == (15, 22)
        back = item['motion_repr_clean'] * ds.Std.astype(np.float64) + ds.Mean
        assert np.abs(back - (g[f'a_item{i}_motion_repr_clean'] * std + mean)).max() <= 2e-6


def test_case_d_sep_noise_items(fx):
    g = fx[0]
    ds = _loader(fx, split='train', task='traj', input_noise=True, sep_noise=True, noise_std_joint=AR.SEP_STD_JOINT, **AR.SEP_STD)
    np.random.seed(int(g['seed_d']))
    mean, std = g['Mean'].astype(np.float64), g['Std'].astype(np.float64)
    for i in range(4):
        item = ds[i]
        assert list(item) == ['motion_repr_clean', 'noisy_joints', 'motion_repr_noisy', 'cond', 'control_cond']
        assert np.abs(item['noisy_joints'] - g[f'd_item{i}_noisy_joints']).max() <= 2.4e-7
        back, ref = item['motion_repr_noisy'] * ds.Std.astype(np.float64) + ds.Mean, g[f'd_item{i}_motion_repr_noisy'] * std + mean
        lim = CR.repr_limits(ref[None], g[f'd_item{i}_noisy_joints'][None].astype(np.float64), None, 2e-6, 4 * 0.0112)[0]
        assert (np.abs(back - ref) <= lim).all()
        assert np.array_equal(item['motion_repr_noisy'][:, 290:], g[f'd_item{i}_motion_repr_noisy'][:, 290:])


def test_joint_widening_measurement():
    """The per-group change of the representation when the noisy joints move by +-5e-6 (the bar of the device's forward
    kinematics), which widens the end-to-end bars of tests/test_gpu_amass_loader.py: re-measured here."""
    g = golden('amass_loader.npz')
    worst = {k: 0.0 for k in AR.JOINT_WIDENING}
    for p, n in (('a_', 4), ('b_', 2)):
        w = AR.joint_widening(g[p + 'joints_noisy'], AR.fixture_params(g, p + 'noisy_', n))
        worst = {k: max(worst[k], w[k]) for k in worst}
    print({k: f'{v:.3e}' for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= AR.JOINT_WIDENING[k] * (1 + 1e-3) and v >= AR.JOINT_WIDENING[k] * (1 - 1e-3), (k, v, AR.JOINT_WIDENING[k])
    # a position moves by what the joints move by; the facing angle by about 2 eps / |across_xy| (0.1 m on this body)
    assert AR.JOINT_WIDENING['root_l_pos'] <= 5e-6 and AR.JOINT_WIDENING['root_rot_angle'] < 2e-4


def test_stats_rule_and_pickles_roundtrip(tmp_path):
    g = golden('amass_loader.npz')
    mean, std = AR.dataset_stats(g['a_repr_clean'])
    ref_mean, ref_std = AR.fixture_stats(g)
    for k in G.REPR_LIST:
        assert np.abs(mean[k] - ref_mean[k]).max() <= float(g['mean_bar']) and np.abs(std[k] - ref_std[k]).max() <= float(g['std_bar'])
    assert (ref_mean['foot_contact'] == 0).all() and (ref_std['foot_contact'] == 1).all()
    assert len(set(ref_std['local_positions'].tolist())) == 1 and len(set(ref_std['smplx_betas'].tolist())) > 1
    assert np.array_equal(np.concatenate([ref_mean[k] for k in ref_mean]), g['Mean'])
    assert pickle.loads(pickle.dumps(ref_mean, protocol=2)).keys() == ref_mean.keys()
