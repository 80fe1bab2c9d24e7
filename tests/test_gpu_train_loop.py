"""GPU: TrainLoopPoseNet / TrainLoopTrajNet (rohm_amd/train/loops.py).
  * With a recording stub for the diffusion the loops reproduce, end to end, the per-step cond and t that the reference's own
    loops recorded (tests/golden/train_loop.npz), and its [test] log lines.
  * With a real 2-layer PoseNet and a real TrajControl net, 6 steps from fixed seeds leave the parameters bitwise equal to a loop
    written out here from the same public pieces (schedule -> training_losses -> backward -> AdamW); the checkpoint of step 4 is
    there and loads strictly; the log lines have the reference's format.
  * A loop fed from a small DataloaderAMASS runs one epoch."""
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import amass_ref as AR
from helpers import PoseDataset, golden
import train_masks_ref as MR
from rohm_amd.train import TrainLoopPoseNet, TrainLoopTrajNet, JsonlWriter
from rohm_amd.train import masks as M
from rohm_amd.train.__main__ import prepare_trajcontrol
from rohm_amd.utils import synth
from test_train_masks_ref import CASES, bank, recorded_cond, seed_all

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LOG_LINE = re.compile(r'^\[Step \d+/ Epoch \d+\] \[(train|test)\]  \w+: -?\d+\.\d{10}$')


class ListLoader:
    def __init__(self, batches, clip_len, traj_feat_dim=22):
        self.batches = batches
        self.dataset = types.SimpleNamespace(clip_len=clip_len, traj_feat_dim=traj_feat_dim)

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        for b in self.batches:
            yield {k: v.clone() for k, v in b.items()}


class Quiet:
    def __init__(self):
        self.lines, self.scalars = [], []

    def info(self, msg):
        self.lines.append(msg)

    def add_scalar(self, tag, value, step):
        self.scalars.append((tag, value, step))


class OneParam(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones((), device=DEV))


class Recorder:
    def __init__(self, traj, num_timesteps):
        self.traj, self.num_timesteps, self.steps, self.evals = traj, num_timesteps, [], []

    def training_losses(self, model, batch, t, noise=None, smplx_model=None, traj_feat_dim=None):
        assert batch['cond'].is_cuda and t.is_cuda
        self.steps.append({'cond': batch['cond'].detach().cpu().numpy(), 't': t.cpu().numpy(),
                           'clean': batch['motion_repr_clean'].detach().cpu().numpy()})
        losses = {'loss': model.w * batch['cond'].abs().mean()}
        return losses if self.traj else (losses, None)

    def eval_losses(self, model, batch, shape, **kw):
        assert kw['compute_loss'] is True
        self.evals.append({'cond': batch['cond'].detach().cpu().numpy(), 'shape': list(shape)})
        return {'loss': torch.tensor(float(len(self.evals)), device=DEV)}, None


def args_for(num_steps, log_interval, save_interval=10 ** 9, bs=3, lr=1e-3):
    return types.SimpleNamespace(batch_size=bs, lr=lr, log_interval=log_interval, save_interval=save_interval, weight_decay=0.0,
                                 body_model_path='unused', num_steps=num_steps, dataset_root='/nowhere/AMASS')


def fixture_batches(gd, prefix, n, traj=False):
    out = []
    for i in range(n):
        b = {k: torch.from_numpy(gd[f'{prefix}{i}_{k}']) for k in ('motion_repr_clean', 'motion_repr_noisy')}
        if traj:
            b['cond'] = b['motion_repr_noisy'][:, :, :22].clone()
        out.append(b)
    return out


@pytest.mark.parametrize('name', list(CASES))
def test_posenet_loop_reproduces_the_recorded_steps(name, tmp_path):
    gd = golden('train_loop.npz')
    case, L = CASES[name], int(gd['clip_len'])
    b = bank(gd)
    b.device = torch.device(DEV)
    rec, quiet = Recorder(False, 1000), Quiet()
    seed_all(int(gd[f'{name}_seed']))
    loop = TrainLoopPoseNet(args_for(int(gd[f'{name}_num_steps']), int(gd[f'{name}_log_interval'])), writer=quiet, model=OneParam(),
                            diffusion_train=rec, diffusion_eval=rec, timestep_respacing_eval='', input_noise=case['input_noise'],
                            train_dataloader=ListLoader(fixture_batches(gd, 'train', 2), L),
                            test_dataloader=ListLoader(fixture_batches(gd, 'test', 1), L), logdir=str(tmp_path), logger=quiet,
                            start_prox_mask_epoch=case['start_prox'], mask_scheme=case['scheme'], device=DEV, prox_bank=b)
    loop.run_loop()
    n = int(gd[f'{name}_n_steps'])
    assert len(rec.steps) == n == loop.step
    for i, st in enumerate(rec.steps):
        assert np.array_equal(st['cond'], recorded_cond(gd, name, i)[1]), (name, i)
        assert np.array_equal(st['t'], gd[f'{name}_t'][i]), (name, i)
        assert np.array_equal(st['clean'].view(np.uint32), MR.transpose(gd[f'train{i % 2}_motion_repr_clean']).view(np.uint32))
    n_eval = len(gd[f'{name}_eval_zero_bits']) if f'{name}_eval_zero_bits' in gd else 0
    assert len(rec.evals) == n_eval
    for i, ev in enumerate(rec.evals):
        assert np.array_equal(ev['cond'], recorded_cond(gd, name, i, 'eval_', 'test0')[1]) and ev['shape'] == [3, 294, 1, 15]
    ref_lines = [str(x) for x in gd[f'{name}_log_lines']]
    assert len(quiet.lines) == len(ref_lines) and all(LOG_LINE.match(x) for x in quiet.lines)
    # one test batch: the mean is the batch's value, so the [test] lines are the reference's to the last digit
    assert [x for x in quiet.lines if '[test]' in x] == [x for x in ref_lines if '[test]' in x]
    assert [x.split(']  ')[0] for x in quiet.lines] == [x.split(']  ')[0] for x in ref_lines]


def test_trajnet_loop_reproduces_the_recorded_steps(tmp_path):
    gd = golden('train_loop.npz')
    rec, quiet = Recorder(True, 100), Quiet()
    seed_all(int(gd['traj_seed']))
    loop = TrainLoopTrajNet(args_for(int(gd['traj_num_steps']), 10 ** 9), writer=None, model=OneParam(), diffusion_train=rec,
                            diffusion_eval=rec, timestep_respacing_eval='', start_infill_epoch=0, max_infill_ratio=0.5,
                            mask_prob=0.6, train_dataloader=ListLoader(fixture_batches(gd, 'train', 2, True), 16, 13),
                            test_dataloader=None, logdir=str(tmp_path), logger=quiet, device=DEV)
    loop.run_loop()
    assert len(rec.steps) == len(gd['traj_cond'])
    for i, st in enumerate(rec.steps):
        assert np.array_equal(st['cond'], gd['traj_cond'][i]) and np.array_equal(st['t'], gd['traj_t'][i]), i


# ---- real networks -----------------------------------------------------------------------------------------------------------------
class Args:
    noise_schedule, sigma_small = 'cosine', True


def _layer():
    from rohm_amd.body_model import SMPLXLayer
    return SMPLXLayer.from_tensors(synth.synthetic_smplx_tensors(0)).to(DEV)


def _posenet(dataset, layer):
    from rohm_amd.model.posenet import PoseNet
    net = PoseNet(dataset, 294, latent_dim=512, ff_size=1024, num_layers=2, num_heads=4, dropout=0.0, traj_feat_dim=22,
                  body_model_path=layer, device=DEV, weight_loss_rec_repr_full_body=1.0, weight_loss_repr_foot_contact_mse=1.0,
                  weight_loss_joint_pos_global=100.0, weight_loss_joint_vel_global=1000.0, weight_loss_joint_smooth=0.0,
                  weight_loss_foot_skating=0.1, start_skating_loss_epoch=0)
    net.load_state_dict(synth.posenet_state_dict(0, num_layers=2), strict=False)
    return net.to(DEV).train()


def _posenet_diffusion(steps=4):
    from rohm_amd.diffusion import gaussian_diffusion_posenet as gdp
    from rohm_amd.diffusion.respace import SpacedDiffusionPoseNet
    from rohm_amd.utils.model_util import create_gaussian_diffusion
    return create_gaussian_diffusion(Args, gdp, SpacedDiffusionPoseNet, steps, '', device=DEV)


def _trajnet_diffusion(steps=4):
    from rohm_amd.diffusion import gaussian_diffusion_trajnet as gdt
    from rohm_amd.diffusion.respace import SpacedDiffusionTrajNet
    from rohm_amd.utils.model_util import create_gaussian_diffusion
    return create_gaussian_diffusion(Args, gdt, SpacedDiffusionTrajNet, steps, '', device=DEV)


def _rows(seed, B, T, mean, std):
    return synth.plausible_motion(seed, B, T, mean, std)[:, :, 0].permute(0, 2, 1).contiguous()      # [B, T, 294]


def _check_run(loop, quiet, logdir, reference_sd, trainable):
    assert loop.step == 6
    sd = {k: v.detach().cpu() for k, v in loop.model.state_dict().items()}
    for k, v in reference_sd.items():
        assert torch.equal(sd[k], v), k                       # bitwise the hand-written loop
    assert all(LOG_LINE.match(x) for x in quiet.lines[:-1]) and quiet.lines[-1] == '[*] model saved\n'
    values = [float(x.rsplit(' ', 1)[1]) for x in quiet.lines[:-1]]
    assert values and np.isfinite(values).all()
    assert {x.split('] [')[1].split(']')[0] for x in quiet.lines[:-1]} == {'train', 'test'}
    assert sorted(f for f in os.listdir(logdir) if f.endswith('.pt')) == ['model000000004.pt']
    ckpt = torch.load(os.path.join(logdir, 'model000000004.pt'), map_location='cpu')
    loop.model.load_state_dict(ckpt, strict=True)
    changed = {k for k in sd if sd[k].is_floating_point() and not torch.equal(sd[k], ckpt[k])}
    assert changed and all(trainable(k) for k in changed)     # steps 5 and 6 moved the trainable weights only


def test_posenet_loop_equals_the_hand_written_loop(tmp_path):
    gd = golden('train_loop.npz')
    B, T, SEED = 4, 15, 31
    mean, std = synth.synthetic_stats(0)
    layer = _layer()
    batches = [{'motion_repr_clean': _rows(20 + i, B, T, mean, std)} for i in range(2)]
    g = torch.Generator().manual_seed(5)
    for b in batches:
        b['motion_repr_noisy'] = b['motion_repr_clean'] + 0.05 * torch.randn(B, T, 294, generator=g)
    test_batches = [{k: v[:2] for k, v in batches[1].items()}]
    make_bank = lambda: M.ProxMaskBank(masks=[gd['prox_mask'].astype(np.float64)], clip_len=16, device=DEV)      # noqa: E731
    args = args_for(num_steps=5, log_interval=2, save_interval=4, bs=B, lr=1e-4)

    # the loop
    seed_all(SEED)
    net, quiet = _posenet(PoseDataset(mean, std), layer), Quiet()
    loop = TrainLoopPoseNet(args, writer=JsonlWriter(str(tmp_path / 'tb')), model=net, diffusion_train=_posenet_diffusion(),
                            diffusion_eval=_posenet_diffusion(), timestep_respacing_eval='', input_noise=True,
                            train_dataloader=ListLoader(batches, 16), test_dataloader=ListLoader(test_batches, 16),
                            logdir=str(tmp_path), logger=quiet, start_prox_mask_epoch=0, mask_scheme='lower+upper+full',
                            device=DEV, prox_bank=make_bank())
    assert loop.num_epochs == 3
    loop.run_loop()

    # the same steps written out
    seed_all(SEED)
    net2, diff, diff_eval = _posenet(PoseDataset(mean, std), layer), _posenet_diffusion(), _posenet_diffusion()
    sched = M.PoseMaskSchedule(0, 'lower+upper+full', True, make_bank())
    opt = torch.optim.AdamW([p for p in net2.parameters() if p.requires_grad], lr=1e-4, weight_decay=0.0)
    step = 0
    for epoch in range(3):
        net2.train()
        for b in batches:
            batch = {k: v.to(DEV) for k, v in b.items()}
            sched(batch, epoch)
            opt.zero_grad()
            t = torch.from_numpy(np.random.choice(4, size=(B,), p=np.ones([4]) / 4)).long().to(DEV)
            losses, _ = diff.training_losses(model=net2, batch=batch, t=t, noise=None, smplx_model=None)
            (losses['loss'] * torch.ones(B, device=DEV)).mean().backward()
            opt.step()
            if step % 2 == 0 and step > 0:
                net2.eval()
                for tb in test_batches:
                    tb = {k: v.to(DEV) for k, v in tb.items()}
                    sched(tb, epoch, eval_block=True)
                    with torch.no_grad():
                        diff_eval.eval_losses(model=net2, batch=tb, shape=list(tb['motion_repr_clean'].shape), progress=False,
                                              clip_denoised=False, cur_epoch=epoch, timestep_respacing='', compute_loss=True)
                net2.train()
            step += 1
    ref_sd = {k: v.detach().cpu() for k, v in net2.state_dict().items()}
    start = synth.posenet_state_dict(0, num_layers=2)
    assert any(not torch.equal(ref_sd[k], start[k]) for k in start if not k.endswith('.pe'))      # it did train
    _check_run(loop, quiet, str(tmp_path), ref_sd, lambda k: not k.startswith('smplx_model.') and not k.endswith('.pe'))
    scalars = [json.loads(x) for x in open(tmp_path / 'tb' / 'scalars.jsonl').read().splitlines()]
    assert {s['tag'].split('/')[0] for s in scalars} == {'train', 'eval'} and {s['step'] for s in scalars} == {2, 4}


def test_trajcontrol_loop_equals_the_hand_written_loop(tmp_path):
    from rohm_amd.model.trajnet import TrajNet
    B, T, SEED = 4, 16, 32
    mean, std = synth.synthetic_stats(0)
    layer = _layer()
    ds = PoseDataset(mean, std)
    ds.traj_feat_dim, ds.clip_len = 13, 17
    weights = dict(weight_loss_root_rec_repr=1.0, weight_loss_root_pos_global=100.0, weight_loss_root_vel_global=1000.0,
                   weight_loss_root_rot_vel_from_abs_traj=1.0, weight_loss_root_smplx_transl_vel=1000.0,
                   weight_loss_root_smplx_rot_vel=1.0, weight_loss_root_smooth=1.0,
                   weight_loss_root_rot_cos_smooth_from_abs_traj=0.0)      # tests/golden/train_cfg/trajnet_ft_trajcontrol.yaml
    g = torch.Generator().manual_seed(6)
    batches = []
    for i in range(2):
        clean = _rows(40 + i, B, T, mean, std)
        batches.append({'motion_repr_clean': clean, 'motion_repr_noisy': clean.clone(),
                        'cond': (clean[..., :13] + 0.1 * torch.randn(B, T, 13, generator=g)).contiguous(),
                        'control_cond': clean[..., -272:].contiguous()})
    test_batches = [{k: v[:2].contiguous() for k, v in batches[0].items()}]
    backbone = synth.trajnet_state_dict(8, trajcontrol=False)

    def make_net():
        net = TrajNet(time_dim=32, mid_dim=512, cond_dim=13, traj_feat_dim=13, trajcontrol=True, device=DEV, dataset=ds,
                      repr_abs_only=True, **weights)
        net.load_state_dict(synth.trajnet_state_dict(9, trajcontrol=True, zero_convs_random=True), strict=True)
        return prepare_trajcontrol(net.to(DEV), backbone)

    class Loader(ListLoader):
        def __init__(self, b):
            self.batches, self.dataset = b, ds
    args = args_for(num_steps=5, log_interval=2, save_interval=4, bs=B, lr=1e-4)

    seed_all(SEED)
    net, quiet = make_net(), Quiet()
    before = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    assert all(torch.equal(before['controlnet.control' + k[4:]], v) for k, v in backbone.items()
               if k.startswith('diff') and 'controlnet.control' + k[4:] in before)
    loop = TrainLoopTrajNet(args, writer=None, model=net, diffusion_train=_trajnet_diffusion(), diffusion_eval=_trajnet_diffusion(),
                            timestep_respacing_eval='', start_infill_epoch=0, max_infill_ratio=0.5, mask_prob=0.6,
                            train_dataloader=Loader(batches), test_dataloader=Loader(test_batches), logdir=str(tmp_path),
                            logger=quiet, device=DEV, smplx_model=layer)
    assert len(loop.opt.param_groups[0]['params']) == sum(1 for k, _ in net.named_parameters() if k.startswith('controlnet.'))
    loop.run_loop()

    seed_all(SEED)
    net2, diff, diff_eval = make_net(), _trajnet_diffusion(), _trajnet_diffusion()
    sched = M.TrajMaskSchedule(0, 0.6, 0.5)
    opt = torch.optim.AdamW([p for p in net2.parameters() if p.requires_grad], lr=1e-4, weight_decay=0.0)
    step = 0
    for epoch in range(3):
        net2.train()
        for b in batches:
            batch = {k: v.clone().to(DEV) for k, v in b.items()}
            sched(batch, epoch, 13)
            opt.zero_grad()
            t = torch.from_numpy(np.random.choice(4, size=(B,), p=np.ones([4]) / 4)).long().to(DEV)
            losses = diff.training_losses(model=net2, batch=batch, t=t, noise=None, traj_feat_dim=13, smplx_model=layer)
            (losses['loss'] * torch.ones(B, device=DEV)).mean().backward()
            opt.step()
            if step % 2 == 0 and step > 0:
                net2.eval()
                for tb in test_batches:
                    tb = {k: v.clone().to(DEV) for k, v in tb.items()}
                    with torch.no_grad():
                        diff_eval.eval_losses(model=net2, batch=tb, shape=[2, T, 13], progress=False, clip_denoised=False,
                                              cur_epoch=epoch, timestep_respacing='', compute_loss=True, smplx_model=layer)
                net2.train()
            step += 1
    ref_sd = {k: v.detach().cpu() for k, v in net2.state_dict().items()}
    _check_run(loop, quiet, str(tmp_path), ref_sd, lambda k: k.startswith('controlnet.'))
    after = {k: v.detach().cpu() for k, v in torch.load(tmp_path / 'model000000004.pt', map_location='cpu').items()}
    moved = {k for k in after if not torch.equal(after[k], before[k])}
    assert moved and all(k.startswith('controlnet.') for k in moved)          # only the control branch learns


def test_loop_fed_from_a_dataloader_amass(tmp_path):
    from rohm_amd.data_loaders.dataloader_amass import DataloaderAMASS
    g = golden('amass_loader.npz')
    root = AR.write_tree(str(tmp_path / 'amass'), AR.fixture_tree(g))
    layer = _layer()
    np.random.seed(int(g['seed_a']))
    kw = dict(preprocessed_amass_root=root, body_model_path=layer, amass_datasets=list(AR.TREE), clip_len=int(g['clip_len']),
              logdir=str(tmp_path / 'log'), device=DEV, task='pose', input_noise=True, **AR.STAGE1_STD)
    os.makedirs(tmp_path / 'log')
    train = DataloaderAMASS(split='train', **kw)
    test = DataloaderAMASS(split='test', spacing=2, **kw)
    seed_all(1)
    net, quiet = _posenet(train, layer), Quiet()
    loop = TrainLoopPoseNet(args_for(num_steps=1, log_interval=1, bs=3, lr=1e-4), writer=None, model=net,
                            diffusion_train=_posenet_diffusion(), diffusion_eval=_posenet_diffusion(), timestep_respacing_eval='',
                            input_noise=True, train_dataloader=train, test_dataloader=test, logdir=str(tmp_path), logger=quiet,
                            start_prox_mask_epoch=10, mask_scheme='lower', device=DEV,
                            generator=torch.Generator().manual_seed(0))
    assert len(train) == 4 and len(loop.train_dataloader) == 2 and loop.num_epochs == 1
    loop.run_loop()
    assert loop.step == 2 and quiet.lines and all(LOG_LINE.match(x) for x in quiet.lines)
    assert np.isfinite([float(x.rsplit(' ', 1)[1]) for x in quiet.lines]).all()
