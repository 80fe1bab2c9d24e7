"""GPU: rohm_amd.drivers.
  * `rohm_result_rows` / `rohm_traj_report` against tests/golden/drivers.npz (the reference scripts' own tails,
    scripts/make_golden_drivers.py): de-normalised representations and per-element report values bit for bit, per-clip sums to 1e-12.
  * The four `*_results` functions on the fixture's inputs: representations bitwise, joints within the bars tests/test_gpu_rederive.py
    holds for the same recoveries (1e-5 m smplx_params / joint_abs_traj, 2e-5 m joint_rel_traj).
  * Each driver end to end through `main(argv)` on the loader tests' synthetic trees with random checkpoints: the written pickle has
    the fixture's keys and dtypes and equals, array for array (torch.equal), what the same seed gives when the loader,
    `run_*_iterations` and the `*_results` function are called by hand; the evaluators read it; `--evaluate` prints their numbers."""
import hashlib
import os
import pickle
import types

import numpy as np
import pytest
import torch

import amass_ref as AR
import drivers_ref as DR
import video_tree as VT
from helpers import golden, max_abs
from rohm_amd import _lib
from rohm_amd.drivers import results as R
from rohm_amd.drivers.__main__ import main, parse_args
from rohm_amd.utils import synth

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BAR = {'smplx_params': 1e-5, 'joint_abs_traj': 1e-5, 'joint_rel_traj': 2e-5}      # tests/test_gpu_rederive.py:107-110


@pytest.fixture(scope='module')
def gd():
    return golden('drivers.npz')


@pytest.fixture(scope='module')
def layer():
    from rohm_amd.body_model import SMPLXLayer
    return SMPLXLayer.from_tensors(synth.synthetic_smplx_tensors(0)).to(DEV)


def dev(d):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in d.items()}


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def dataset(st, traj_feat_dim=22):
    return types.SimpleNamespace(Mean=st[0], Std=st[1], traj_feat_dim=traj_feat_dim, pose_feat_dim=272)


# ---- rohm_result_rows ---------------------------------------------------------------------------------------------------------------
def test_result_rows_small_both_layouts(gd):
    """B = 2, T = 15: partial tiles on both axes (15 < 32, 294 = 9 * 32 + 6), rows of 15 floats."""
    st = DR.stats()
    inp = dev(DR.amass_inputs(0, st))
    ref = [gd['amass_full_save_' + k][:2] for k in ('motion_repr_clean_list', 'motion_repr_rec_list', 'motion_repr_noisy_list')]
    got = R.result_rows([(inp['clean'], 'bc1t'), (inp['rec'], 'bc1t'), (inp['noisy'], 'btc', inp['traj_noisy_full'])], st)
    assert all(g.shape == (2, 15, 294) and g.dtype == torch.float32 and g.is_contiguous() for g in got)
    assert all(same_bits(g, r) for g, r in zip(got, ref))
    # the other layout of every source, and the noisy rows without the override
    noisy_cm = inp['noisy'].permute(0, 2, 1).contiguous().unsqueeze(2)
    got = R.result_rows([(DR.rows(inp['clean']), 'btc'), (noisy_cm, 'bc1t', inp['traj_noisy_full']), (inp['noisy'], 'btc')], st)
    assert same_bits(got[0], ref[0]) and same_bits(got[1], ref[2])
    assert same_bits(got[2], DR.denorm(inp['noisy'].cpu().numpy(), *st))
    assert not same_bits(got[2][:, :, :22], ref[2][:, :, :22]) and same_bits(got[2][:, :, 22:], ref[2][:, :, 22:])


def test_result_rows_large(gd):
    """B = 3, T = 143: rows that are only 4-byte aligned, more than one tile on both axes, the first T rows of a longer tensor."""
    st = DR.stats()
    inp = dev(DR.rows_large_inputs(st))
    assert inp['noisy'].shape == (3, 144, 294)
    got = R.result_rows([(inp['clean'], 'bc1t'), (inp['rec'], 'bc1t'), (inp['noisy'], 'btc', inp['traj_noisy_full'])], st, T=143)
    plain, = R.result_rows([(inp['noisy'], 'btc')], st, T=143)
    assert all(g.shape == (3, 143, 294) for g in got + [plain])
    host = DR.amass_denorm({k: v.cpu() for k, v in inp.items()}, st, 143)
    for g, h in zip(got, host):
        assert same_bits(g, h)
    assert [sha(g) for g in got + [plain]] == [str(s) for s in gd['rows_large_sha']]
    # four sources: two launches
    four = R.result_rows([(inp['clean'], 'bc1t')] * 4, st)
    assert len(four) == 4 and all(torch.equal(f, got[0]) for f in four)


def test_result_rows_refuses_bad_arguments():
    import ctypes as C
    st = DR.stats()
    x = torch.zeros(2, 294, 1, 15, device=DEV)
    with pytest.raises(_lib.RohmHipError, match='CPU'):
        R.result_rows([(x.cpu(), 'bc1t')], st)
    with pytest.raises(_lib.RohmHipError, match='at least T=15'):
        R.result_rows([(x, 'bc1t', torch.zeros(2, 14, 22, device=DEV))], st)
    with pytest.raises(ValueError):
        R.result_rows([(x, 'btc')], st)
    with pytest.raises(ValueError):
        R.result_rows([(x, 'bc1t'), (torch.zeros(2, 10, 294, device=DEV), 'btc')], st)
    lib = _lib.lib()
    stream = _lib.stream_ptr(torch.device(DEV))
    assert lib.rohm_result_rows(None, 1, 2, 15, 294, stream) == -1            # ROHM_ERR_ARG
    item = (_lib.ResultRowsItem * 1)()
    out = torch.empty(2, 15, 294, device=DEV)
    mean = torch.zeros(294, device=DEV)
    item[0].src, item[0].stride_b, item[0].stride_t, item[0].stride_c = None, 294 * 15, 1, 15
    item[0].mean, item[0].std, item[0].out = mean.data_ptr(), mean.data_ptr(), out.data_ptr()
    assert lib.rohm_result_rows(item, 1, 2, 15, 294, stream) == -1 and b'null pointer' in lib.rohm_last_error()
    item[0].src = x.data_ptr()
    assert lib.rohm_result_rows(item, 4, 2, 15, 294, stream) == -1
    item[0].stride_t, item[0].stride_c = 2, 30                                  # neither axis contiguous
    assert lib.rohm_result_rows(item, 1, 2, 15, 294, stream) == -1
    assert C.sizeof(_lib.ResultRowsItem) == 72


# ---- rohm_traj_report ---------------------------------------------------------------------------------------------------------------
def _report_inputs(gd, tag, T):
    joints = []
    for k in DR.JOINT_NAMES:
        j = np.concatenate([gd[f'trajnet_{tag}_b{i}_joints_{k}'] for i in range(2)])
        full = np.zeros((j.shape[0], T, 22, 3), np.float32)
        full[:, :, :j.shape[2]] = j                                             # T = 144: the fixture holds the pelvis only
        joints.append(torch.from_numpy(full).to(DEV))
    reprs = []
    for k in ('clean', 'rec'):
        r = torch.zeros(joints[0].shape[0], T, 294, device=DEV)
        r[:, :, 0] = torch.from_numpy(np.concatenate([gd[f'trajnet_{tag}_b{i}_rot_{k}'] for i in range(2)])).to(DEV)
        reprs.append(r)
    return joints, reprs


@pytest.mark.parametrize('tag,T', [('t16', 16), ('t144', 144)])
def test_traj_report_vs_the_script(gd, tag, T):
    joints, (rc, rr) = _report_inputs(gd, tag, T)
    rep, elems = R.traj_report(joints, rc, rr, return_elems=True)
    assert elems.shape == (3, 15, T) and rep.sums.shape == (3, 15) and rep.clip_len == T
    assert same_bits(elems[:, :10], gd[f'trajnet_{tag}_elems_err'])
    assert same_bits(elems[:, 10:, :T - 3], gd[f'trajnet_{tag}_elems_jitter'])
    assert float(elems[:, 10:, T - 3:].abs().max()) == 0.0
    ref = gd[f'trajnet_{tag}_sums']
    assert (np.abs(rep.sums - ref) <= 1e-12 * np.abs(ref)).all()
    rep2, elems2 = R.traj_report(joints, rc, rr, return_elems=True)
    assert np.array_equal(rep.sums.view(np.uint64), rep2.sums.view(np.uint64)) and torch.equal(elems, elems2)
    assert np.array_equal(R.traj_report(joints, rc, rr).sums.view(np.uint64), rep.sums.view(np.uint64))
    # the lines agree with the script's wherever its float32 means are not within float32 accuracy of a rounding boundary
    assert rep.lines()[0] == str(gd[f'trajnet_{tag}_lines'][0]) and len(rep.lines()) == 6


def test_traj_report_refuses_short_clips():
    j = [torch.zeros(2, 3, 22, 3, device=DEV)] * 5
    r = torch.zeros(2, 3, 294, device=DEV)
    with pytest.raises(_lib.RohmHipError, match=r'code -1.*T >= 4'):
        R.traj_report(j, r, r)
    with pytest.raises(_lib.RohmHipError, match='CPU'):
        R.traj_report([t.cpu() for t in j], r, r)
    with pytest.raises(ValueError):
        R.traj_report(j[:4], r, r)
    j4 = [torch.zeros(2, 4, 22, 3, device=DEV)] * 5
    assert R.traj_report(j4, torch.zeros(2, 4, 294, device=DEV), torch.zeros(2, 4, 294, device=DEV)).sums.shape == (2, 15)


# ---- the four tails -----------------------------------------------------------------------------------------------------------------
def _check(res, ref_of, n_rows, modes):
    for k, v in res.items():
        if not isinstance(v, torch.Tensor):
            continue
        ref = ref_of(k)
        assert v.shape == ref.shape and v.dtype == torch.float32, k
        if k in modes:
            err = max_abs(v.cpu(), torch.from_numpy(ref))
            print(f'{k}: max |joint error| {err:.3e} m (bar {BAR[modes[k]]:.0e})')
            assert err < BAR[modes[k]], k
        else:
            assert same_bits(v, ref), k
    return n_rows


AMASS_MODES = {'rec_ric_data_clean_list': 'smplx_params', 'rec_ric_data_noisy_list': 'smplx_params',
               'rec_ric_data_rec_list_from_abs_traj': 'joint_abs_traj', 'rec_ric_data_rec_list_from_smpl': 'smplx_params'}


def test_amass_full_results(gd, layer):
    st = DR.stats()
    a = 0
    for i, n in enumerate(DR.BATCHES):
        inp = dev(DR.amass_inputs(i, st))
        res = R.amass_full_results(inp['rec'], {'motion_repr_clean': inp['clean'], 'motion_repr_noisy': inp['noisy']},
                                   inp['traj_noisy_full'], dataset(st), layer, True)
        assert list(res) == [str(k) for k in gd['amass_full_save_keys']][3:]
        _check(res, lambda k: gd['amass_full_save_' + k][a:a + n], n, AMASS_MODES)
        a += n
    res = R.amass_full_results(inp['rec'], {'motion_repr_clean': inp['clean']}, None, dataset(st), layer, False)
    assert not [k for k in res if 'noisy' in k] and len(res) == 5


def test_posenet_results(gd, layer):
    st = DR.stats()
    a = 0
    for i, n in enumerate(DR.BATCHES):
        inp = dev(DR.posenet_inputs(i, st))
        res = R.posenet_results(inp['rec'], {'motion_repr_clean': inp['clean'], 'motion_repr_noisy': inp['noisy']}, dataset(st), layer)
        assert res['motion_repr_rec_list'].shape == (n, 16, 294)
        host = {k: v.cpu().numpy() for k, v in res.items()}
        if i == 0:
            R.threshold_contact_labels(host)          # the recorded file has batch 0 thresholded (test_posenet.py:260-265)
        _check({k: torch.from_numpy(v) for k, v in host.items()}, lambda k: gd['posenet_save_' + k][a:a + n], n, AMASS_MODES)
        a += n


@pytest.mark.parametrize('name', ['prox', 'egobody'])
def test_prox_egobody_results(gd, layer, name):
    st = DR.stats()
    modes = {'rec_ric_data_noisy_list': 'smplx_params', 'rec_ric_data_rec_list_from_abs_traj': 'joint_abs_traj',
             'rec_ric_data_rec_list_from_smpl': 'smplx_params'}
    a = 0
    for i, n in enumerate(DR.BATCHES):
        inp = dev(DR.prox_inputs(i, st, name))
        batch = {'motion_repr_noisy': inp['noisy'], 'frame_name': inp['frame_name'], 'transf_matrix': inp['transf_matrix'],
                 'noisy_joints_scene_coord': inp['noisy_joints_scene_coord'], 'gt_joints_scene_coord': inp['gt_joints_scene_coord'],
                 'mask_joint_vis': inp['mask_joint_vis']}
        res = R.prox_egobody_results(inp['rec'], batch, dataset(st), layer, name)
        static = ('repr_name_list', 'repr_dim_dict', 'recording_name', 'gender_gt')
        assert list(res) == [k for k in (str(x) for x in gd[f'{name}_save_keys']) if k not in static]
        assert res['mask_joint_vis_list'].shape == (n, 15, 22) and (res['frame_name_list'] == inp['frame_name']).all()
        _check(res, lambda k: gd[('egobody' if k == 'joints_gt_scene_coord_list' else 'prox') + '_save_' + k][a:a + n], n, modes)
        a += n
    with pytest.raises(ValueError):
        R.prox_egobody_results(inp['rec'], batch, dataset(st), layer, 'amass')


def test_trajnet_results_and_report(gd, layer):
    st = DR.stats()
    body_t = synth.synthetic_smplx_tensors(0)
    modes = {'rec_ric_data_clean': 'smplx_params', 'rec_ric_data_noisy': 'smplx_params', 'rec_ric_data_rec_from_abs_traj': 'joint_abs_traj',
             'rec_ric_data_rec_from_rel_traj': 'joint_rel_traj', 'rec_ric_data_rec_from_smpl': 'smplx_params'}
    report = None
    for i, n in enumerate(DR.BATCHES):
        inp = dev(DR.trajnet_inputs(i, st, 16, body_t))
        res = R.trajnet_results(inp['val_output'], {'motion_repr_clean': inp['clean'], 'motion_repr_noisy': inp['noisy']},
                                dataset(st, 13), layer, True)
        for k, mode in modes.items():
            ref = gd[f'trajnet_t16_b{i}_joints_' + k[len('rec_ric_data_'):]]
            err = max_abs(res[k].cpu(), torch.from_numpy(ref))
            print(f'{k}: max |joint error| {err:.3e} m (bar {BAR[mode]:.0e})')
            assert err < BAR[mode], k
        assert same_bits(res['motion_repr_clean'][:, :, 0], gd[f'trajnet_t16_b{i}_rot_clean'])
        assert same_bits(res['motion_repr_clean_root_rec'][:, :, 0], gd[f'trajnet_t16_b{i}_rot_rec'])
        if i == 0:
            for k in ('clean', 'root_noisy', 'root_rec'):
                assert same_bits(res['motion_repr_clean' + ('' if k == 'clean' else '_' + k)], gd['trajnet_t16_b0_repr_' + k]), k
        m = R.traj_report([res[k] for k in modes], res['motion_repr_clean'], res['motion_repr_clean_root_rec'])
        report = m if report is None else report.merge(m)
    # the report of the device joints against the script's means, as far as the joints' bars e carry: an error term |a - b| moves by
    # at most 2 e; a jitter component (weights 1, 3, 3, 1, times 27000) by 8 e 27000, its norm by sqrt(3) times that
    means = gd['trajnet_t16_means'].astype(np.float64)
    got = np.array(list(report.summary().values()))
    e = BAR['joint_rel_traj']
    assert np.abs(got[:10] - means[:10]).max() < 2 * e + 1e-6 * np.abs(means[:10]).max()
    assert np.abs(got[10:] - means[10:]).max() < 3 ** 0.5 * 8 * e * 27000 + 1e-6 * np.abs(means[10:]).max()
    assert report.lines()[0] == '[EVAL] 3 clips in total.'


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def body_dir(tmp_path_factory):
    """SMPLX_NEUTRAL.npz in the released layout (posedirs [V, 3, 486], kintree_table, weights) from the synthetic model."""
    t = synth.synthetic_smplx_tensors(0)
    V = t['v_template'].shape[0]
    kt = np.stack([np.array(synth.SMPLX_PARENTS), np.arange(55)]).astype(np.int64)
    kt[0, 0] = 2 ** 32 - 1
    d = tmp_path_factory.mktemp('body')
    for name in ('SMPLX_NEUTRAL.npz', 'SMPLX_FEMALE.npz'):
        np.savez(str(d / name), v_template=t['v_template'].numpy(), shapedirs=t['shapedirs'].numpy(),
                 posedirs=t['posedirs'].numpy().T.reshape(V, 3, 486), J_regressor=t['J_regressor'].numpy(), kintree_table=kt,
                 weights=t['lbs_weights'].numpy(), f=np.zeros((4, 3), np.int64))
    return str(d)


def _stats_pickles(logdir, mean_dict, std_dict):
    os.makedirs(logdir, exist_ok=True)
    for name, d in (('AMASS_mean.pkl', mean_dict), ('AMASS_std.pkl', std_dict)):
        with open(os.path.join(logdir, name), 'wb') as f:
            pickle.dump(d, f, protocol=2)


def _checkpoints(logdir, which=('posenet', 'trajnet', 'control')):
    os.makedirs(logdir, exist_ok=True)
    sd = {'posenet': lambda: synth.posenet_state_dict(0), 'trajnet': lambda: synth.trajnet_state_dict(1, trajcontrol=False),
          'control': lambda: synth.trajnet_state_dict(2, trajcontrol=True)}
    out = {}
    for k in which:
        out[k] = os.path.join(logdir, f'model_{k}.pt')
        torch.save(sd[k](), out[k])
    return out


@pytest.fixture(scope='module')
def amass_tree(tmp_path_factory):
    """The loader tests' tree under the names the drivers read (TCDHands, TotalCapture, SFU) plus one sequence: at clip_len 17 the
    test split has 2 + 1 + 1 = 4 clips."""
    g = golden('amass_loader.npz')
    arrays = {}
    for key, v in AR.fixture_tree(g).items():
        arrays[key.replace('SetA', 'TCDHands').replace('SetB', 'SFU')] = v
    jw, world = synth.synthetic_recording(34, 21, 'z')
    joints, smplx = np.zeros((21, 25, 3), np.float32), np.zeros((21, 178))
    joints[:, :22], smplx[:, :79] = jw, world
    arrays['TotalCapture/more'] = (joints, smplx)
    root = AR.write_tree(str(tmp_path_factory.mktemp('amass')), arrays)
    logdir = str(tmp_path_factory.mktemp('ckpt'))
    _stats_pickles(logdir, *AR.fixture_stats(g))
    return root, logdir, _checkpoints(logdir)


SMALL = ['--clip_len', '17', '--batch_size', '2']


def _load_pickle(path):
    with open(path, 'rb') as f:
        return pickle.load(f)


def _check_pickle(gd, got, prefix):
    assert list(got) == [str(k) for k in gd[f'{prefix}_save_keys']]
    for k, t in zip(gd[f'{prefix}_save_keys'], gd[f'{prefix}_save_dtypes']):
        v = got[str(k)]
        assert (str(v.dtype) if isinstance(v, np.ndarray) and str(k) != 'frame_name_list' else type(v).__name__) == \
            (str(t) if str(k) != 'frame_name_list' else 'ndarray'), k


def test_amass_full_end_to_end(gd, amass_tree, body_dir, tmp_path, capsys):
    from rohm_amd.data_loaders.dataloader_amass import DataloaderAMASS
    from rohm_amd.drivers import __main__ as M
    from rohm_amd.evaluation import amass_lines, evaluate_amass
    from rohm_amd.inference import run_amass_iterations
    root, logdir, ck = amass_tree
    argv = ['amass_full', '--dataset_root', root, '--body_model_path', body_dir, '--model_path_posenet', ck['posenet'],
            '--model_path_trajnet', ck['trajnet'], '--model_path_trajnet_control', ck['control'], '--diffusion_steps_posenet', '6',
            '--diffusion_steps_trajnet', '4', '--sample_iter', '2', '--load_noise', 'False', '--mask_scheme', 'lower',
            '--save_root', str(tmp_path / 'res'), '--seed', '5', '--evaluate'] + SMALL
    out = main(argv)
    printed = capsys.readouterr().out
    args = parse_args('amass_full', argv[1:])
    assert out['path'] == R.amass_full_pickle_path(args) and os.path.basename(out['path']) == \
        'test_amass_full_grad_True_mask_lower_iter_2_iter2trajnoisy_True_iter2posenoisy_True_earlystop_False_seed_5.pkl'
    got = _load_pickle(out['path'])
    _check_pickle(gd, got, 'amass_full')
    # 4 clips at batch size 2: three steps, the first batch a second time
    assert got['motion_repr_rec_list'].shape == (6, 15, 294) and got['rec_ric_data_clean_list'].shape == (6, 15, 22, 3)
    assert np.array_equal(got['motion_repr_clean_list'][4:6], got['motion_repr_clean_list'][0:2])
    assert not np.array_equal(got['motion_repr_rec_list'][4:6], got['motion_repr_rec_list'][0:2])      # sampled again, new noise

    # the same seed by hand
    M.fixseed(5)
    body = M._make_body_model(body_dir, DEV)
    kw = dict(preprocessed_amass_root=root, split='test', amass_datasets=M.TEST_DATASETS, body_model_path=body, input_noise=True,
              noise_std_smplx_global_rot=3.0, noise_std_smplx_body_rot=3.0, noise_std_smplx_trans=0.03, noise_std_smplx_betas=0.1,
              load_noise=False, loaded_smplx_noise_dict=None, clip_len=17, device=DEV)
    pose_ds = DataloaderAMASS(task='pose', logdir=logdir, **kw)
    traj_ds = DataloaderAMASS(task='traj', repr_abs_only=True, logdir=logdir, **kw)
    assert len(pose_ds) == 4
    models, diffusions = M._two_stage(args, pose_ds, traj_ds, body, DEV)
    pose_batches, traj_batches = list(pose_ds.batches(2)), list(traj_ds.batches(2))
    parts = []
    for k in R.step_schedule(4, 2):
        bp, bt = pose_ds._assemble(torch.arange(2 * k, 2 * k + 2, device=DEV)), traj_ds._assemble(torch.arange(2 * k, 2 * k + 2, device=DEV))
        assert all(torch.equal(bp[key], pose_batches[k][key]) for key in bp)
        noisy_traj = bt['motion_repr_noisy'][:, :, 0:22].clone()
        vp, _, _ = run_amass_iterations(args, models, diffusions, bt, bp, traj_ds, pose_ds, body)
        parts.append(R.amass_full_results(vp, bp, noisy_traj, pose_ds, body, True))
    for key in parts[0]:
        hand = torch.cat([p[key] for p in parts]).cpu()
        assert torch.equal(torch.from_numpy(got[key]), hand), key
    assert len(traj_batches) == 2
    # the evaluator reads the file; --evaluate printed the same numbers from the device results
    lines = amass_lines(evaluate_amass(out['path'], 'lower', 0.0, DEV))
    assert out['lines'] == lines and all(ln in printed for ln in lines)


def test_posenet_and_trajnet_end_to_end(gd, amass_tree, body_dir, capsys):
    from rohm_amd.drivers import __main__ as M
    root, logdir, ck = amass_tree
    common = ['--dataset_root', root, '--body_model_path', body_dir, '--seed', '2'] + SMALL
    # ---- posenet: T = 16 frames (17 tokens), two batches, 'full' mask drawn from the host generator
    argv = ['posenet', '--model_path', ck['posenet'], '--diffusion_steps', '6', '--mask_scheme', 'full', '--save_results', 'True',
            '--evaluate'] + common
    out = main(argv)
    printed = capsys.readouterr().out
    assert 'interactive viewer is not part of the package' in printed
    assert out['path'] == os.path.join(logdir, 'test_posenet_model_posenet_guidance_False.pkl')
    got = _load_pickle(out['path'])
    _check_pickle(gd, got, 'posenet')
    assert got['motion_repr_rec_list'].shape == (4, 16, 294)
    assert set(np.unique(got['motion_repr_rec_list'][:2, :, -4:])) <= {0.0, 1.0}          # test_posenet.py:260-265
    assert not set(np.unique(got['motion_repr_rec_list'][2:, :, -4:])) <= {0.0, 1.0}
    assert out['lines'] and all(ln.startswith('[EVAL] ') and ln in printed for ln in out['lines'])
    # by hand
    args = parse_args('posenet', argv[1:])
    M.fixseed(2)
    body = M._make_body_model(body_dir, DEV)
    ds = M._amass_dataset(args, body, DEV, repr_abs_only=False)
    model = M._posenet(args, ds, body, DEV, ck['posenet'], strict=False)
    diff = M._diffusion(args, 'posenet', 6, DEV)
    parts = []
    for batch in ds.batches(2):
        cond = batch['motion_repr_noisy'].clone()
        start = torch.FloatTensor(2).uniform_(0, 16 - 1).long()
        from rohm_amd.inference import apply_occlusion_mask
        apply_occlusion_mask(cond, 'full', 22, start, torch.clamp(start + 30, max=16))
        batch['motion_repr_clean'] = batch['motion_repr_clean'].permute(0, 2, 1).unsqueeze(-2)
        batch['cond'] = cond.permute(0, 2, 1).unsqueeze(-2)
        _, vo = diff.eval_losses(model=model, batch=batch, shape=[2, 294, 1, 16], progress=False, clip_denoised=False,
                                 timestep_respacing='', cond_fn_with_grad=False, smplx_model=body)
        parts.append({k: v.cpu().numpy() for k, v in R.posenet_results(vo, batch, ds, body, True).items()})
    R.threshold_contact_labels(parts[0])
    for key in parts[0]:
        assert np.array_equal(got[key], np.concatenate([p[key] for p in parts])), key

    # ---- trajnet: prints the script's report
    argv = ['trajnet', '--model_path', ck['trajnet'], '--diffusion_steps', '4', '--infill_traj', 'True', '--max_infill_ratio', '0.5',
            '--visualize', 'False'] + common
    out = main(argv)
    printed = capsys.readouterr().out
    assert 'interactive viewer' not in printed
    assert out['report'].n_clips == 4 and out['report'].clip_len == 16
    assert out['lines'][0] == '[EVAL] 4 clips in total.' and len(out['lines']) == 6 and all(ln in printed for ln in out['lines'])
    args = parse_args('trajnet', argv[1:])
    M.fixseed(2)
    ds = M._amass_dataset(args, body, DEV, repr_abs_only=True)
    model = M._trajnet(args, ds, DEV, ck['trajnet'], False)
    diff = M._diffusion(args, 'trajnet', 4, DEV)
    report = None
    for batch in ds.batches(2):
        batch['cond'][:, :, 0:13] = batch['cond'][:, :, 0:13] * M.traj_infill_window(2, 16, 0.5, 13, DEV)
        _, vo = diff.eval_losses(model=model, batch=batch, shape=[2, 16, 13], progress=False, clip_denoised=False,
                                 timestep_respacing='', cond_fn_with_grad=False, compute_loss=False, smplx_model=body)
        res = R.trajnet_results(vo, batch, ds, body, True)
        m = R.traj_report([res['rec_ric_data_' + k] for k in DR.JOINT_NAMES], res['motion_repr_clean'], res['motion_repr_clean_root_rec'])
        report = m if report is None else report.merge(m)
    assert np.array_equal(report.sums.view(np.uint64), out['report'].sums.view(np.uint64))


def test_traj_infill_window_is_the_scripts_loop():
    """test_trajnet.py:139-148 draws start and length from the host generator and zeroes mask[bs, start:end] in a loop."""
    from rohm_amd.drivers.__main__ import traj_infill_window
    torch.manual_seed(11)
    got = traj_infill_window(5, 16, 0.9, 13, DEV).cpu()
    torch.manual_seed(11)
    start = torch.FloatTensor(5).uniform_(0, 16 - 1).long()
    end = start + (16 * torch.FloatTensor(5).uniform_(0, 1) * 0.9).long()
    end[end > 16] = 16
    ref = torch.ones(5, 16)
    for b in range(5):
        ref[b, start[b]:end[b]] = 0
    assert torch.equal(got, ref.unsqueeze(-1).repeat(1, 1, 13)) and 0 < float(ref.mean()) < 1


@pytest.fixture(scope='module')
def scene_trees(tmp_path_factory):
    """The video loader tests' synthetic PROX / EgoBody recordings, 50 frames long: three clips at clip_len 17, overlap 2."""
    n = VT.N_FRAMES
    VT.N_FRAMES = 50
    out = {}
    try:
        for name in ('prox', 'egobody'):
            a = VT.synthetic_tree_arrays(name, seed=3)
            paths = VT.write_tree(str(tmp_path_factory.mktemp(name)), name, a)
            out[name] = (a, paths, _checkpoints(paths['logdir']))
    finally:
        VT.N_FRAMES = n
    return out


@pytest.mark.parametrize('name', ['prox', 'egobody'])
def test_prox_egobody_end_to_end(gd, scene_trees, body_dir, tmp_path, capsys, name):
    from rohm_amd.data_loaders.dataloader_video import DataloaderVideo
    from rohm_amd.drivers import __main__ as M
    from rohm_amd.evaluation import evaluate_scene
    from rohm_amd.inference import run_prox_iterations
    a, paths, ck = scene_trees[name]
    rec, scene = str(a['recording_name']), str(a['scene_name'])
    floors = tmp_path / 'floors.json'
    floors.write_text('{"%s": -0.05}' % (scene if name == 'prox' else rec))          # by scene, or by recording as the evaluator's
    argv = ['prox_egobody', '--dataset', name, '--dataset_root', paths['base_dir'], '--init_root', paths['init_root'],
            '--recording_name', rec, '--body_model_path', body_dir, '--model_path_posenet', ck['posenet'], '--model_path_trajnet',
            ck['trajnet'], '--model_path_trajnet_control', ck['control'], '--diffusion_steps_posenet', '6',
            '--diffusion_steps_trajnet', '4', '--sample_iter', '2', '--save_root', str(tmp_path / 'res'), '--seed', '4',
            '--floor_heights', str(floors), '--save_interval', '1', '--evaluate'] + SMALL
    out = main(argv)
    printed = capsys.readouterr().out
    args = parse_args('prox_egobody', argv[1:])
    assert out['path'] == R.prox_egobody_pickle_path(args, rec) and out['path'].endswith(
        f'test_{name}_grad_True_iter_2_iter2trajnoisy_False_iter2posenoisy_False_earlystop_True_seed_4/' + rec + '.pkl')
    got = _load_pickle(out['path'])
    _check_pickle(gd, got, name)
    assert got['motion_repr_rec_list'].shape == (3, 15, 294) and got['mask_joint_vis_list'].shape == (3, 15, 22)
    assert got['frame_name_list'].shape == (1, 17) and got['recording_name'] == rec          # the last batch's names only
    if name == 'egobody':
        assert got['gender_gt'] == 'female' and got['joints_gt_scene_coord_list'].shape == (3, 17, 22, 3)
    # by hand
    M.fixseed(4)
    body = M._make_body_model(body_dir, DEV)
    kw = dict(dataset=name, init_root=paths['init_root'], base_dir=paths['base_dir'], body_model_path=body_dir, recording_name=rec,
              use_scene_floor_height=True, clip_len=17, overlap_len=2, device=DEV, floor_heights={scene: -0.05})
    pose_ds = DataloaderVideo(task='pose', logdir=paths['logdir'], **kw)
    traj_ds = DataloaderVideo(task='traj', repr_abs_only=True, logdir=paths['logdir'], **kw)
    assert len(pose_ds) == 3 and R.step_schedule(3, 2) == [0, 1]
    models, diffusions = M._two_stage(args, pose_ds, traj_ds, body, DEV)
    parts = []
    for bp, bt in zip(pose_ds.batches(2), traj_ds.batches(2)):
        vj, _, _ = run_prox_iterations(args, models, diffusions, bt, bp, traj_ds, pose_ds, body)
        parts.append(R.prox_egobody_results(vj, bp, pose_ds, body, name))
    for key in parts[0]:
        if key == 'frame_name_list':
            assert (got[key] == parts[-1][key]).all()
        else:
            assert torch.equal(torch.from_numpy(got[key]), torch.cat([p[key] for p in parts]).cpu()), key
    # the evaluator reads the file; --evaluate printed the same numbers from the device results
    per = evaluate_scene(name, os.path.dirname(out['path']), [rec], {rec: -0.05}, DEV)
    assert per[rec].lines() == out['lines'] and all(ln in printed for ln in out['lines'][1:])
    assert np.array_equal(per[rec].sums, out['report'].sums, equal_nan=True)
