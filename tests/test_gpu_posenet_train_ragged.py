"""GPU: PoseNet's training path at ragged token counts.  include/rohm_hip.h takes 1 <= T <= 144, the other training tests run
S = T + 1 in {64, 144, 145} only.  softmax_fwd_kernel / softmax_bwd_kernel cover a row in three 64-key chunks predicated on j < S:
here a row ends inside the first chunk (S = 2, 3, 16, 17), just past it (65), inside the second (101) and just past that (129);
T % 4 != 0 (1, 2, 15, 100 is not, 16 / 64 / 128 are multiples) moves the strided in-place reads of [B, C, 1, T].  The method and
the bars of tests/test_gpu_posenet_train.py: forward, input gradients and every parameter gradient against torch autograd of the
oracle network in float64, no worse than 8x torch's own float32 autograd (check_against), with and without the five dropouts."""
import math

import pytest
import torch

from oracle import nets
from test_gpu_posenet_train import (DEV, check_against, device_grads, fetch_masks, inputs, make_net, ref_grads)

pytestmark = pytest.mark.gpu
TRAJ = 22


def report(label, worst):
    k = max(worst, key=lambda n: worst[n][0])
    print(f'{label} worst gradient {k}: rel {worst[k][0]:.3e} (torch float32 {worst[k][1]:.3e})')


@pytest.mark.parametrize('L,B,T', [(1, 3, 1), (1, 2, 2), (1, 5, 15), (1, 3, 16), (1, 2, 64), (1, 3, 100), (1, 2, 128),
                                   (2, 3, 16), (2, 2, 100)])
def test_gradients_match_float64_autograd(L, B, T):
    net, sd = make_net(L)
    x, c, t, cot = inputs(B, T, seed=30 + T)
    dev = device_grads(net, x, c, t, cot)
    assert dev[0].shape == (B, 294, 1, T) and set(dev[1]) == {k for k in sd if not k.endswith('.pe')}
    assert torch.equal(dev[0][:, :TRAJ], c[:, :TRAJ])          # the trajectory channels are cond's, copied
    worst = check_against(dev, ref_grads(sd, x, c, t, cot, torch.float64), ref_grads(sd, x, c, t, cot, torch.float32))
    report(f'[L={L},B={B},S={T + 1}]', worst)


@pytest.mark.parametrize('B,T', [(2, 16), (2, 64), (3, 100)])
def test_dropout_matches_masked_float64_and_reproduces(B, T):
    """The attention dropout's mask index is row * S + j: a stride slip would pair probabilities with another key's mask bit."""
    L, p = 2, 0.1
    net, sd = make_net(L, dropout=p)
    x, c, t, cot = inputs(B, T, seed=50 + T)
    torch.manual_seed(321)
    dev = device_grads(net, x, c, t, cot)
    seed = net.last_dropout_seed
    masks = fetch_masks(seed, L, B, T, p)
    assert masks[(0, 1)].shape == (B, 4, T + 1, T + 1)
    assert torch.equal(dev[0][:, :TRAJ], c[:, :TRAJ])
    worst = check_against(dev, ref_grads(sd, x, c, t, cot, torch.float64, masks, p), ref_grads(sd, x, c, t, cot, torch.float32, masks, p))
    report(f'[dropout,B={B},S={T + 1}]', worst)
    for key, mk in masks.items():      # keep fraction of every site within 5 sigma of 1 - p (the smallest mask has 2 x 4 x 17 x 17 bits)
        frac = mk.double().mean().item()
        assert abs(frac - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / mk.numel()), (key, frac)
    torch.manual_seed(321)
    dev2 = device_grads(net, x, c, t, cot)
    assert net.last_dropout_seed == seed
    assert torch.equal(dev[0], dev2[0]) and torch.equal(dev[2], dev2[2]) and torch.equal(dev[3], dev2[3])
    assert all(torch.equal(dev[1][k], dev2[1][k]) for k in dev[1])


def test_train_forward_equals_inference_forward_at_101_tokens():
    net, sd = make_net(8)
    x, c, t, _ = inputs(3, 100, seed=7)
    batch = {'x_t': x.to(DEV), 'cond': c.to(DEV)}
    out_train = net(batch, t.to(DEV))
    assert out_train.grad_fn is not None
    with torch.no_grad():
        out_eval = net.eval()(batch, t.to(DEV))
    ref = nets.posenet_forward(sd, x, c, t, dtype=torch.float64)
    e_te = float((out_train.detach() - out_eval).abs().max())
    e_t, e_e = float((out_train.detach().cpu() - ref).abs().max()), float((out_eval.cpu() - ref).abs().max())
    print(f'train-vs-eval {e_te:.3e}  train-vs-f64 {e_t:.3e}  eval-vs-f64 {e_e:.3e}')
    assert e_te <= 1e-5
    assert e_t < 1e-4 and e_e < 1e-4          # the bar of the committed golden (tests/test_gpu_posenet.py)
