"""GPU: the training loops with optimizer='native' (rohm_amd.optim.AdamW).
  * 2-layer PoseNet, 6 steps from fixed seeds: the parameters' deviation from a float64-optimiser run of the hand-written loop is at
    most 4 x the deviation of the same loop under torch's fp32 optimiser from it (optim_ref's measure and margin); the step-4
    checkpoint is there and loads strictly; the log lines have the reference's format.
    (Measured on an MI355X: 2.89 for the native loop, 1.37 for torch's; Adam's update is a sign for near-zero gradients, so a few
    small weights move by whole steps under rounding noise in either run.)
  * TrajControl fine-tune via prepare_trajcontrol: only controlnet.* tensors move, every backbone tensor keeps its bits, the optimiser
    holds exactly the controlnet.* parameters.
  * Without the option the loop's optimiser is torch.optim.AdamW."""
import os

import numpy as np
import pytest
import torch

import optim_ref as R
import test_gpu_train_loop as TL
from helpers import PoseDataset, golden
from rohm_amd import optim
from rohm_amd.train import TrainLoopPoseNet, TrainLoopTrajNet
from rohm_amd.train import masks as M
from rohm_amd.train.__main__ import prepare_trajcontrol
from rohm_amd.utils import synth
from test_train_masks_ref import seed_all

pytestmark = pytest.mark.gpu
DEV = TL.DEV


def _args(optimizer=None, **kw):
    args = TL.args_for(num_steps=5, log_interval=2, save_interval=4, bs=4, lr=1e-4)
    if optimizer is not None:
        args.optimizer = optimizer
    for k, v in kw.items():
        setattr(args, k, v)
    return args


def test_posenet_loop_with_the_native_optimiser(tmp_path):
    gd = golden('train_loop.npz')
    B, T, SEED = 4, 15, 31
    mean, std = synth.synthetic_stats(0)
    layer = TL._layer()
    batches = [{'motion_repr_clean': TL._rows(20 + i, B, T, mean, std)} for i in range(2)]
    g = torch.Generator().manual_seed(5)
    for b in batches:
        b['motion_repr_noisy'] = b['motion_repr_clean'] + 0.05 * torch.randn(B, T, 294, generator=g)
    test_batches = [{k: v[:2] for k, v in batches[1].items()}]
    make_bank = lambda: M.ProxMaskBank(masks=[gd['prox_mask'].astype(np.float64)], clip_len=16, device=DEV)      # noqa: E731

    def run_loop(optimizer, logdir):
        seed_all(SEED)
        net, quiet = TL._posenet(PoseDataset(mean, std), layer), TL.Quiet()
        os.makedirs(logdir, exist_ok=True)
        loop = TrainLoopPoseNet(_args(optimizer), writer=None, model=net, diffusion_train=TL._posenet_diffusion(),
                                diffusion_eval=TL._posenet_diffusion(), timestep_respacing_eval='', input_noise=True,
                                train_dataloader=TL.ListLoader(batches, 16), test_dataloader=TL.ListLoader(test_batches, 16),
                                logdir=logdir, logger=quiet, start_prox_mask_epoch=0, mask_scheme='lower+upper+full', device=DEV,
                                prox_bank=make_bank())
        loop.run_loop()
        return loop, quiet

    loop, quiet = run_loop('native', str(tmp_path / 'native'))
    assert type(loop.opt) is optim.AdamW and loop.opt.max_grad_norm is None
    loop_t, _ = run_loop(None, str(tmp_path / 'torch'))
    assert type(loop_t.opt) is torch.optim.AdamW

    # the hand-written loop with the optimiser in float64: master copies take the step, the net gets them rounded to fp32
    seed_all(SEED)
    net2, diff, diff_eval = TL._posenet(PoseDataset(mean, std), layer), TL._posenet_diffusion(), TL._posenet_diffusion()
    sched = M.PoseMaskSchedule(0, 'lower+upper+full', True, make_bank())
    named = [(k, p) for k, p in net2.named_parameters() if p.requires_grad]
    masters = [p.detach().double().clone().requires_grad_() for _, p in named]
    opt = torch.optim.AdamW(masters, lr=1e-4, weight_decay=0.0)
    step = 0
    for epoch in range(3):
        net2.train()
        for b in batches:
            batch = {k: v.to(DEV) for k, v in b.items()}
            sched(batch, epoch)
            for _, p in named:
                p.grad = None
            t = torch.from_numpy(np.random.choice(4, size=(B,), p=np.ones([4]) / 4)).long().to(DEV)
            losses, _ = diff.training_losses(model=net2, batch=batch, t=t, noise=None, smplx_model=None)
            (losses['loss'] * torch.ones(B, device=DEV)).mean().backward()
            for mp, (_, p) in zip(masters, named):
                mp.grad = None if p.grad is None else p.grad.double()
            opt.step()
            with torch.no_grad():
                for mp, (_, p) in zip(masters, named):
                    p.copy_(mp)
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
    r64 = {k: mp.detach().cpu() for (k, _), mp in zip(named, masters)}
    start = synth.posenet_state_dict(0, num_layers=2)
    assert any(not torch.equal(r64[k].float(), start[k]) for k in r64 if k in start)                 # it did train

    def deviation(lp):
        sd = dict(lp.model.named_parameters())
        return max(R.tensor_error(sd[k].detach().double().cpu(), r64[k]) for k in r64)
    own, bar = deviation(loop), deviation(loop_t)
    print('native loop deviation', own, 'torch fp32 loop deviation', bar)
    assert own <= R.MARGIN * bar, (own, bar)
    TL._check_run(loop, quiet, str(tmp_path / 'native'), {}, lambda k: not k.startswith('smplx_model.') and not k.endswith('.pe'))


def test_trajcontrol_fine_tune_with_the_native_optimiser(tmp_path):
    from rohm_amd.model.trajnet import TrajNet
    B, T, SEED = 4, 16, 32
    mean, std = synth.synthetic_stats(0)
    layer = TL._layer()
    ds = PoseDataset(mean, std)
    ds.traj_feat_dim, ds.clip_len = 13, 17
    weights = dict(weight_loss_root_rec_repr=1.0, weight_loss_root_pos_global=100.0, weight_loss_root_vel_global=1000.0,
                   weight_loss_root_rot_vel_from_abs_traj=1.0, weight_loss_root_smplx_transl_vel=1000.0,
                   weight_loss_root_smplx_rot_vel=1.0, weight_loss_root_smooth=1.0,
                   weight_loss_root_rot_cos_smooth_from_abs_traj=0.0)
    g = torch.Generator().manual_seed(6)
    batches = []
    for i in range(2):
        clean = TL._rows(40 + i, B, T, mean, std)
        batches.append({'motion_repr_clean': clean, 'motion_repr_noisy': clean.clone(),
                        'cond': (clean[..., :13] + 0.1 * torch.randn(B, T, 13, generator=g)).contiguous(),
                        'control_cond': clean[..., -272:].contiguous()})
    backbone = synth.trajnet_state_dict(8, trajcontrol=False)
    net = TrajNet(time_dim=32, mid_dim=512, cond_dim=13, traj_feat_dim=13, trajcontrol=True, device=DEV, dataset=ds,
                  repr_abs_only=True, **weights)
    net.load_state_dict(synth.trajnet_state_dict(9, trajcontrol=True, zero_convs_random=True), strict=True)
    net = prepare_trajcontrol(net.to(DEV), backbone)

    class Loader(TL.ListLoader):
        def __init__(self, b):
            self.batches, self.dataset = b, ds
    seed_all(SEED)
    before = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    args = _args('native', max_grad_norm=1.0)
    args.num_steps, args.save_interval = 2, 10 ** 9
    loop = TrainLoopTrajNet(args, writer=None, model=net, diffusion_train=TL._trajnet_diffusion(),
                            diffusion_eval=TL._trajnet_diffusion(), timestep_respacing_eval='', start_infill_epoch=0,
                            max_infill_ratio=0.5, mask_prob=0.6, train_dataloader=Loader(batches), test_dataloader=None,
                            logdir=str(tmp_path), logger=TL.Quiet(), device=DEV, smplx_model=layer)
    assert type(loop.opt) is optim.AdamW and loop.opt.max_grad_norm == 1.0
    control = {k: p for k, p in net.named_parameters() if k.startswith('controlnet.')}
    held = [p for grp in loop.opt.param_groups for p in grp['params']]
    assert len(held) == len(control) and {id(p) for p in held} == {id(p) for p in control.values()}
    loop.run_loop()
    assert loop.step == 4
    after = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    moved = {k for k in after if not torch.equal(after[k], before[k])}
    assert moved and all(k.startswith('controlnet.') for k in moved)
    bits = lambda x: x.contiguous().reshape(-1).view(torch.uint8)      # noqa: E731
    assert all(torch.equal(bits(after[k]), bits(before[k])) for k in after if not k.startswith('controlnet.'))
    assert set(loop.opt.state) <= set(control.values()) and len(loop.opt.state) > 0
    assert bool(torch.isfinite(loop.opt.last_grad_norm)) and all(bool(torch.isfinite(v).all()) for v in after.values())


def test_the_default_optimiser_is_torchs(tmp_path):
    gd = golden('train_loop.npz')
    rec = TL.Recorder(False, 1000)
    loop = TrainLoopPoseNet(TL.args_for(1, 10 ** 9), writer=None, model=TL.OneParam(), diffusion_train=rec, diffusion_eval=rec,
                            timestep_respacing_eval='', input_noise=True,
                            train_dataloader=TL.ListLoader(TL.fixture_batches(gd, 'train', 2), int(gd['clip_len'])),
                            test_dataloader=None, logdir=str(tmp_path), logger=None, start_prox_mask_epoch=10,
                            mask_scheme='lower', device=DEV)
    assert type(loop.opt) is torch.optim.AdamW
    with pytest.raises(ValueError, match='max_grad_norm needs'):
        TrainLoopPoseNet(_args(None, max_grad_norm=1.0), writer=None, model=TL.OneParam(), diffusion_train=rec, diffusion_eval=rec,
                         timestep_respacing_eval='', input_noise=True,
                         train_dataloader=TL.ListLoader(TL.fixture_batches(gd, 'train', 2), int(gd['clip_len'])),
                         test_dataloader=None, logdir=str(tmp_path), logger=None, start_prox_mask_epoch=10, mask_scheme='lower',
                         device=DEV)
