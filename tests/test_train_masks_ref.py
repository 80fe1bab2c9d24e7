"""CPU: the training loops' host side against tests/golden/train_loop.npz, the steps the reference's own
TrainLoopPoseNet.run_loop / TrainLoopTrajNet.run_loop recorded (scripts/make_golden_train_loop.py):
  * the numpy restatement of the mask rules (tests/train_masks_ref.py) rebuilds every recorded cond;
  * the host schedules of rohm_amd.train.masks, re-seeded, make the recorded decisions (joint sets, windows, PROX clips over
    successive shuffles) and, with the loop's np.random.choice, the recorded t;
  * the PROX bank's ratio filter and bit packing; the config reader on the six training configs; prepare_trajcontrol."""
import os
import random

import numpy as np
import pytest
import torch

from helpers import golden
import train_masks_ref as MR
from rohm_amd.train import masks as M
from rohm_amd.train.__main__ import parse_args, prepare_trajcontrol, read_config

CFG_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'train_cfg')
BRANCHES = ['joints', 'prox', 'lower', 'upper', 'full', 'none']
CASES = {'p1n': dict(input_noise=True, start_prox=10 ** 6, scheme='lower'),
         'p1c': dict(input_noise=False, start_prox=10 ** 6, scheme='lower'),
         'p2a': dict(input_noise=True, start_prox=-1, scheme='lower+upper+full'),
         'p2l': dict(input_noise=True, start_prox=-1, scheme='lower')}


@pytest.fixture(scope='module')
def gd():
    return golden('train_loop.npz')


def seed_all(seed):
    random.seed(seed)
    torch.manual_seed(seed)
    np.random.seed(seed)


def recorded_cond(gd, name, i, prefix='', batch=None):
    """The recorded cond of step i: the transposed source rows with 0 where the fixture's bits say the loop's cond differed."""
    key = 'motion_repr_noisy' if CASES[name]['input_noise'] else 'motion_repr_clean'
    src = gd[f'{batch or "train%d" % (i % 2)}_{key}']
    zero = np.unpackbits(gd[f'{name}_{prefix}zero_bits'][i])[:src.size].reshape(src.shape).astype(bool)
    return src, np.where(MR.transpose(zero), np.float32(0), MR.transpose(src))


def bank(gd):
    return M.ProxMaskBank(masks=[gd['prox_mask'].astype(np.float64)], clip_len=int(gd['clip_len']), device='cpu')


def decision_kwargs(gd, name, i, bits):
    b = BRANCHES[int(gd[f'{name}_branch'][i])]
    kw = dict(zero_contact=bool(gd[f'{name}_zero_contact'][i]))
    if b in ('joints', 'lower', 'upper'):
        kw['joint_bits'] = gd[f'{name}_joint_bits'][i]
    if b == 'full':
        kw['window'] = gd[f'{name}_window'][i]
    if b == 'prox':
        kw.update(vis_bits=bits, vis_index=gd[f'{name}_vis_index'][i])
    return b, kw


@pytest.mark.parametrize('name', list(CASES))
def test_restatement_rebuilds_every_recorded_cond(gd, name):
    bits = bank(gd).bits_host
    for i in range(int(gd[f'{name}_n_steps'])):
        src, cond = recorded_cond(gd, name, i)
        _, kw = decision_kwargs(gd, name, i, bits)
        assert np.array_equal(MR.train_cond(src, **kw), cond), (name, i)
    if f'{name}_eval_zero_bits' in gd:
        for i in range(len(gd[f'{name}_eval_zero_bits'])):
            src, cond = recorded_cond(gd, name, i, 'eval_', 'test0')
            got = MR.train_cond(src, joint_bits=gd[f'{name}_eval_joint_bits'][i], zero_contact=CASES[name]['input_noise'])
            assert np.array_equal(got, cond), (name, 'eval', i)


def test_restatement_rebuilds_the_trajnet_cond(gd):
    for i in range(len(gd['traj_cond'])):
        src = gd[f'train{i % 2}_motion_repr_noisy'][:, :, :22]
        assert np.array_equal(MR.traj_window(src, gd['traj_window'][i], 13), gd['traj_cond'][i]), i
        assert bool(gd['traj_masked'][i]) == bool((gd['traj_window'][i][:, 1] > gd['traj_window'][i][:, 0]).any())


def test_fixture_covers_the_branches(gd):
    b = [BRANCHES[int(x)] for x in gd['p2a_branch']]
    assert set(b) == {'prox', 'lower', 'upper', 'full'}
    ups = [MR.joints_of(gd['p2a_joint_bits'][i][0]) for i in range(len(b)) if b[i] == 'upper']
    assert any(21 in u for u in ups) and any(u == sorted(MR.UPPER) for u in ups)
    assert any((gd['p2a_window'][i][:, 1] == 15).any() for i in range(len(b)) if b[i] == 'full')
    for name in ('p1n', 'p1c'):
        bits = gd[f'{name}_joint_bits'].reshape(-1)
        assert (bits & MR.bits_of((7, 10))).any() and (bits & MR.bits_of((8, 11))).any() and not (bits & 1).any()


@pytest.mark.parametrize('name', list(CASES))
def test_posenet_schedule_reproduces_the_decisions(gd, name):
    case, bs, T = CASES[name], int(gd['bs']), int(gd['clip_len']) - 1
    sched = M.PoseMaskSchedule(case['start_prox'], case['scheme'], case['input_noise'], bank(gd))
    seed_all(int(gd[f'{name}_seed']))
    log_interval, n_eval = int(gd[f'{name}_log_interval']), 0
    for step in range(int(gd[f'{name}_n_steps'])):
        d = sched.decide(step // 2, bs, T)
        t = np.random.choice(1000, size=(bs,), p=np.ones([1000]) / 1000)
        assert d.branch == BRANCHES[int(gd[f'{name}_branch'][step])], (step, d.branch)
        assert d.zero_contact == bool(gd[f'{name}_zero_contact'][step])
        if d.joint_bits is not None:
            assert np.array_equal(d.joint_bits, gd[f'{name}_joint_bits'][step]), step
        if d.window is not None:
            assert np.array_equal(d.window, gd[f'{name}_window'][step]), step
        if d.vis_index is not None:
            assert np.array_equal(d.vis_index, gd[f'{name}_vis_index'][step]), step
        assert np.array_equal(t, gd[f'{name}_t'][step]), step
        if step % log_interval == 0 and step > 0:
            e = sched.decide_eval(bs)
            assert np.array_equal(e.joint_bits, gd[f'{name}_eval_joint_bits'][n_eval])
            n_eval += 1
    assert n_eval == (len(gd[f'{name}_eval_zero_bits']) if f'{name}_eval_zero_bits' in gd else 0)


def test_phase1_never_hides_the_pelvis_and_remaps_joint_zero():
    sched = M.PoseMaskSchedule(10, 'lower', True)
    seed_all(3)
    drawn_zero = False
    for _ in range(50):
        state = torch.get_rng_state()
        d = sched.decide(0, 4, 15)
        torch.set_rng_state(state)
        raw = (torch.rand(4, len(d.joints[0])) * 22).long()
        drawn_zero |= bool((raw == 0).any())
        expect = raw.clone()
        expect[expect == 0] = 1
        assert d.joints == expect.tolist() and not (d.joint_bits & 1).any()
    assert drawn_zero


def test_trajnet_schedule_reproduces_the_decisions(gd):
    bs, T = int(gd['bs']), int(gd['clip_len']) - 1
    sched = M.TrajMaskSchedule(0, 0.6, 0.5)
    seed_all(int(gd['traj_seed']))
    for step in range(len(gd['traj_cond'])):
        d = sched.decide(step // 2, bs, T)
        t = np.random.choice(100, size=(bs,), p=np.ones([100]) / 100)
        assert (d.window is not None) == bool(gd['traj_masked'][step]) or \
            (d.window is not None and not (d.window[:, 1] > d.window[:, 0]).any()), step
        if d.window is not None:
            # a window of length 0 leaves no trace in the recorded cond: compare the masks the windows stand for
            src = gd[f'train{step % 2}_motion_repr_noisy'][:, :, :22]
            assert np.array_equal(MR.traj_window(src, d.window, 13), gd['traj_cond'][step]), step
            live = d.window[:, 1] > d.window[:, 0]
            assert np.array_equal(d.window[live], gd['traj_window'][step][live]), step
        assert np.array_equal(t, gd['traj_t'][step]), step
    assert M.TrajMaskSchedule(5, 1.0, 0.5).decide(4, bs, T).window is None      # before start_infill_epoch: no draw, no mask


def test_prox_bank_filter_packing_and_shuffle(gd):
    mask, L = gd['prox_mask'].astype(np.float64), int(gd['clip_len'])
    b = bank(gd)
    kept = gd['prox_kept']
    assert len(b) == len(kept) == 10 and 2 not in kept and 7 not in kept        # ratio 0 and 4 / 352 < 0.05
    for k, i in enumerate(kept):
        clip = mask[i * L:(i + 1) * L]
        assert np.array_equal(b.bits_host[k], MR.pack_visibility(clip))
        assert np.array_equal(((b.bits_host[k][:, None] >> np.arange(22, dtype=np.uint32)) & 1), clip[:, :22].astype(np.uint32))
    # the threshold itself: 18 of 352 hidden is kept (0.0511), 17 is not (0.0483)
    for hidden, keep in ((18, 1), (17, 0)):
        m = np.ones((L, 25))
        m.reshape(-1)[[f * 25 + j for f in range(L) for j in range(22)][:hidden]] = 0
        assert len(M.pack_prox_clips([m], L)) == keep
    with pytest.raises(ValueError, match='only 0 and 1'):
        M.pack_prox_clips([np.full((L, 22), 0.5)], L)
    # the order vector follows np.random.shuffle of the clip array itself, cumulatively
    arr = np.arange(10)[:, None].repeat(3, axis=1).astype(np.float64)
    np.random.seed(5)
    want = []
    for _ in range(4):
        np.random.shuffle(arr)
        want.append(arr[:3, 0].astype(np.int64).copy())
    np.random.seed(5)
    got = [b.draw(3) for _ in range(4)]
    assert all(np.array_equal(w, g) for w, g in zip(want, got))
    with pytest.raises(ValueError, match='cannot fill a batch'):
        b.draw(11)


def test_prox_bank_reads_a_sorted_tree(tmp_path, gd):
    L = int(gd['clip_len'])
    rng = np.random.RandomState(0)
    arrays = {}
    for name in ('N3OpenArea_00157_01', 'BasementSittingBooth_00142_01', 'MPH11_00034_01'):
        arrays[name] = (rng.rand(2 * L + 3, 25) > 0.3).astype(np.float64)
        os.makedirs(tmp_path / 'PROX' / 'mask_joint' / name)
        np.save(tmp_path / 'PROX' / 'mask_joint' / name / 'mask_joint.npy', arrays[name])
    b = M.ProxMaskBank(str(tmp_path), clip_len=L, device='cpu')
    assert b.recordings == sorted(arrays)
    assert np.array_equal(b.bits_host, M.pack_prox_clips([arrays[k] for k in sorted(arrays)], L)) and len(b) == 6


def test_schedule_refusals(gd):
    with pytest.raises(ValueError, match='mask_scheme'):
        M.PoseMaskSchedule(0, 'upper', True)
    seed_all(0)
    sched = M.PoseMaskSchedule(-1, 'lower', True, None)
    with pytest.raises(ValueError, match='ProxMaskBank'):
        for _ in range(50):
            sched.decide(0, 3, 15)
    with pytest.raises(ValueError, match='cannot fill a batch'):
        s2 = M.PoseMaskSchedule(-1, 'lower', True, bank(gd))
        for _ in range(50):
            s2.decide(0, 11, 15)


# ---- the drivers' arguments ----------------------------------------------------------------------------------------------------
def test_config_reader_on_the_training_configs():
    files = sorted(os.listdir(CFG_DIR))
    assert files == ['posenet_train_stage1.yaml', 'posenet_train_stage2.yaml', 'trajnet_ft_trajcontrol.yaml',
                     'trajnet_train_vanilla_stage1.yaml', 'trajnet_train_vanilla_stage2.yaml', 'trajnet_train_vanilla_stage3.yaml']
    raw = read_config(os.path.join(CFG_DIR, 'posenet_train_stage2.yaml'))
    assert raw['pretrained_model_path'] == 'runs/63369/model000300000.pt' and raw['save_dir'] == 'runs' and raw['lr'] == '1e-4'
    a = parse_args('posenet', ['--config', os.path.join(CFG_DIR, 'posenet_train_stage2.yaml')])
    assert (a.diffusion_steps, a.clip_len, a.batch_size, a.start_prox_mask_epoch) == (1000, 145, 64, 500)
    assert a.mask_scheme == 'lower+upper+full' and a.load_pretrained_model is True and a.input_noise is True and a.debug is False
    assert a.lr == 1e-4 and isinstance(a.lr, float) and a.noise_std_smplx_trans == 0.03 and a.weight_loss_foot_skating == 0.1
    assert a.timestep_respacing_eval == '' and a.num_steps == 1000000000 and isinstance(a.num_steps, int) and a.sigma_small is True
    a1 = parse_args('posenet', ['--config', os.path.join(CFG_DIR, 'posenet_train_stage1.yaml'), '--batch_size', '8', '--debug', 'True'])
    assert a1.batch_size == 8 and a1.debug is True and a1.task == 'pose' and a1.load_pretrained_model is False
    t = parse_args('trajnet', ['--config', os.path.join(CFG_DIR, 'trajnet_ft_trajcontrol.yaml')])
    assert t.trajcontrol is True and t.load_pretrained_backbone is True and t.load_pretrained_model is False
    assert t.pretrained_backbone_path == 'runs/79530/model000450000.pt' and t.repr_abs_only is True and t.diffusion_steps == 100
    assert t.start_infill_epoch == 100000000000000000000 and t.mask_prob == 0.4 and t.max_infill_ratio == 0.1
    assert t.weight_loss_root_pos_global == 100.0 and isinstance(t.weight_loss_root_pos_global, float)
    for f in files[3:]:
        v = parse_args('trajnet', ['--config', os.path.join(CFG_DIR, f)])
        assert v.task == 'traj' and v.trajcontrol is False and isinstance(v.start_infill_epoch, int) and v.batch_size >= 1
    # defaults without a file are the drivers'
    d = parse_args('trajnet', [])
    assert (d.diffusion_steps, d.batch_size, d.noise_std_smplx_trans, d.trajcontrol) == (100, 64, 0.02, False)
    p = parse_args('posenet', [])
    assert (p.diffusion_steps, p.batch_size, p.noise_std_smplx_trans, p.mask_scheme) == (1000, 32, 0.01, 'lower')


def test_config_reader_refuses_what_it_cannot_read(tmp_path):
    bad = tmp_path / 'bad.yaml'
    bad.write_text('lr 1e-4\n')
    with pytest.raises(ValueError, match='expected `key: value`'):
        read_config(str(bad))
    bad.write_text('learning_rate: 1e-4\n')
    with pytest.raises(ValueError, match='unknown settings'):
        parse_args('posenet', ['--config', str(bad)])
    bad.write_text("save_dir: 'runs # not a comment'  # a comment\nmask_scheme: upper\n")
    assert read_config(str(bad))['save_dir'] == 'runs # not a comment'
    with pytest.raises(ValueError, match='mask_scheme must be one of'):
        parse_args('posenet', ['--config', str(bad)])


def test_prepare_trajcontrol_copies_and_freezes():
    from rohm_amd.model.trajnet import TrajNet
    torch.manual_seed(0)
    backbone = TrajNet(time_dim=32, mid_dim=64, cond_dim=13, traj_feat_dim=13, trajcontrol=False)
    bsd = {k: v.clone() for k, v in backbone.state_dict().items()}
    torch.manual_seed(1)
    model = TrajNet(time_dim=32, mid_dim=64, cond_dim=13, traj_feat_dim=13, trajcontrol=True)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    prepare_trajcontrol(model, bsd)
    sd = model.state_dict()
    copied = 0
    for k, v in bsd.items():
        assert torch.equal(sd[k], v), k                                       # the backbone itself
        if k.startswith('diff'):
            tgt = 'controlnet.control' + k[4:]
            if tgt in sd:
                assert torch.equal(sd[tgt], v), tgt
                copied += 1
    assert copied > 20
    untouched = [k for k in sd if k.startswith('controlnet.') and 'zero_conv' in k]
    assert untouched and all(torch.equal(sd[k], before[k]) for k in untouched)
    for name, p in model.named_parameters():
        assert p.requires_grad == name.startswith('controlnet.'), name
    assert model.training and model.controlnet.training
    assert not model.diff_enc1.training and not model.cond_enc1.training and not model.time_mlp.training
    # without a backbone: only the freeze
    m2 = TrajNet(time_dim=32, mid_dim=64, cond_dim=13, traj_feat_dim=13, trajcontrol=True)
    w = {k: v.clone() for k, v in m2.state_dict().items()}
    prepare_trajcontrol(m2)
    assert all(torch.equal(v, w[k]) for k, v in m2.state_dict().items())
    assert {n.split('.')[0] for n, p in m2.named_parameters() if p.requires_grad} == {'controlnet'}
