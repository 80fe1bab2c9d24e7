"""GPU: PoseNet's training path at the shipped clip length, clip_len 145 = T 144 frames = 145 tokens (the length of
cfg_files/train_cfg/posenet_train_stage*.yaml and of test_posenet.py).  The method and the bars of tests/test_gpu_posenet_train.py:
forward, input gradients and every parameter gradient against torch autograd of the oracle network in float64, with and without the
five dropouts (their masks from rohm_posenet_dropout_mask); two runs bitwise equal; T = 145 still refused; one TrainLoopPoseNet
step on 144-frame batches with a PROX mask bank of clip_len 144.  145 tokens make every per-clip size odd (the 145 x 145 attention
slabs, a weight-gradient slice of 576 rows that ends inside a clip), which the 144-token tests never see."""
import numpy as np
import pytest
import torch

from rohm_amd import _lib
from rohm_amd.utils import synth
from test_gpu_posenet_train import (DEV, check_against, device_grads, fetch_masks, inputs, make_net, ref_grads)

pytestmark = pytest.mark.gpu
B, T = 2, 144


@pytest.mark.parametrize('L', [1, 2])
def test_gradients_match_float64_autograd_at_144_frames(L):
    net, sd = make_net(L)
    x, c, t, cot = inputs(B, T, seed=21)
    dev = device_grads(net, x, c, t, cot)
    assert dev[0].shape == (B, 294, 1, T) and set(dev[1]) == {k for k in sd if not k.endswith('.pe')}
    check_against(dev, ref_grads(sd, x, c, t, cot, torch.float64), ref_grads(sd, x, c, t, cot, torch.float32))
    dev2 = device_grads(net, x, c, t, cot)
    assert torch.equal(dev[0], dev2[0]) and torch.equal(dev[2], dev2[2]) and torch.equal(dev[3], dev2[3])
    assert all(torch.equal(dev[1][k], dev2[1][k]) for k in dev[1])


@pytest.mark.parametrize('L', [1, 2])
def test_dropout_matches_masked_float64_at_144_frames(L):
    p = 0.1
    net, sd = make_net(L, dropout=p)
    x, c, t, cot = inputs(B, T, seed=22)
    torch.manual_seed(77)
    dev = device_grads(net, x, c, t, cot)
    seed = net.last_dropout_seed
    masks = fetch_masks(seed, L, B, T, p)
    assert masks[(0, 1)].shape == (B, 4, T + 1, T + 1)
    check_against(dev, ref_grads(sd, x, c, t, cot, torch.float64, masks, p), ref_grads(sd, x, c, t, cot, torch.float32, masks, p))
    torch.manual_seed(77)
    dev2 = device_grads(net, x, c, t, cot)
    assert net.last_dropout_seed == seed
    assert torch.equal(dev[0], dev2[0]) and all(torch.equal(dev[1][k], dev2[1][k]) for k in dev[1])


def test_more_rows_than_one_weight_gradient_slice():
    """B = 5: 725 token rows, two weight-gradient slices, the first of which ends inside the fourth clip."""
    net, sd = make_net(1)
    x, c, t, cot = inputs(5, T, seed=23)
    dev = device_grads(net, x, c, t, cot)
    check_against(dev, ref_grads(sd, x, c, t, cot, torch.float64), ref_grads(sd, x, c, t, cot, torch.float32))


def test_145_frames_are_still_refused():
    net, _ = make_net(1)
    long_x = torch.randn(1, 294, 1, 145, device=DEV)
    with pytest.raises(_lib.RohmHipError, match=r'T=145.*1 <= T <= 144'):
        net({'x_t': long_x, 'cond': long_x}, torch.zeros(1, dtype=torch.int64, device=DEV))


def test_train_loop_step_at_144_frames(tmp_path):
    from helpers import PoseDataset
    from rohm_amd.train import TrainLoopPoseNet
    from rohm_amd.train import masks as M
    from test_gpu_train_loop import (LOG_LINE, ListLoader, Quiet, _layer, _posenet, _posenet_diffusion, _rows, args_for)
    from test_train_masks_ref import seed_all
    mean, std = synth.synthetic_stats(0)
    batches = [{'motion_repr_clean': _rows(60 + i, B, T, mean, std)} for i in range(2)]
    g = torch.Generator().manual_seed(8)
    for b in batches:
        b['motion_repr_noisy'] = b['motion_repr_clean'] + 0.05 * torch.randn(B, T, 294, generator=g)
    rng = np.random.RandomState(3)
    bank = M.ProxMaskBank(masks=[(rng.rand(3 * 144 + 7, 25) > 0.2).astype(np.float64)], clip_len=144, device=DEV)
    assert len(bank) == 3
    seed_all(4)          # random.uniform draws 0.236, 0.103, ...: the first steps take the PROX branch
    net, quiet = _posenet(PoseDataset(mean, std), _layer()), Quiet()
    loop = TrainLoopPoseNet(args_for(num_steps=1, log_interval=1, bs=B, lr=1e-4), writer=None, model=net,
                            diffusion_train=_posenet_diffusion(), diffusion_eval=_posenet_diffusion(), timestep_respacing_eval='',
                            input_noise=True, train_dataloader=ListLoader(batches, 145), test_dataloader=ListLoader(batches[:1], 145),
                            logdir=str(tmp_path), logger=quiet, start_prox_mask_epoch=-1, mask_scheme='lower', device=DEV,
                            prox_bank=bank)
    branches = []
    decide = loop.schedule.decide
    loop.schedule.decide = lambda *a, **k: branches.append(decide(*a, **k)) or branches[-1]
    before = {k: v.detach().clone() for k, v in net.named_parameters()}
    loop.run_loop()
    assert loop.step == 2 and [d.branch for d in branches] == ['prox', 'prox']
    assert quiet.lines and all(LOG_LINE.match(x) for x in quiet.lines)          # the eval block ran eval_losses at T = 144
    assert {x.split('] [')[1].split(']')[0] for x in quiet.lines} == {'train', 'test'}
    assert np.isfinite([float(x.rsplit(' ', 1)[1]) for x in quiet.lines]).all()
    moved = [k for k, v in net.named_parameters() if v.requires_grad and not torch.equal(v.detach(), before[k])]
    assert moved
