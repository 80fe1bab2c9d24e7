"""GPU: TrajNet / TrajControl away from the drivers' (traj_feat_dim 13, control_cond_dim 272, T 144): every width and clip length
include/rohm_hip.h documents (1 <= c_traj <= 32, c_ctrl <= 320, T a multiple of 16 up to 512) through the inference forward, both
forms of the sampling loop (launch per layer, clip-resident), the training forward and backward, and the refusals just outside.
The reference's other released configuration, repr_abs_only=False, has traj_feat_dim 22; width 32 fills the head's LDS staging
([c_traj][65] in traj_tail_kernel, [c_traj][hcin + 1] in the resident step) and leaves no pad column in the 32-wide rows; T = 512
is the GroupNorm limit of both paths (8 channels x 512 frames = 256 threads x 16 values) and makes one clip (516 padded rows)
longer than a weight-gradient slab of the training path (kSlabRows = 512), T = 256 cuts the slabs differently per level (1, 3,
7, 14, 25 clips per slab).  Methods and bars are those of tests/test_gpu_trajnet.py and tests/test_gpu_trajnet_train.py."""
import pytest
import torch

from helpers import cpu_noise_sequence, max_abs, seeded
from oracle import diffusion as odiff
from oracle import nets
from rohm_amd import _lib
from test_gpu_trajnet import _loop, make_diffusion, make_trajnet
from test_gpu_trajnet_train import (REL_BAR, check_all, device_grads, freeze_backbone, inputs, make_net, ref_grads, rel)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
STEPS = 10      # sampling steps of the loop tests: the bars were set for 100 steps, ten accumulate less error

_FWD64 = {}


def weight_seed(ct, ctrl):
    return 300 + 2 * ct + int(ctrl)


def forward64(case, sd, x, c, k, t):
    """The float64 oracle forward of a case, computed once per module run and shared (read only)."""
    if case not in _FWD64:
        _FWD64[case] = nets.trajnet_forward(sd, x, c, t, control_cond=k if case[2] else None, dtype=torch.float64)
    return _FWD64[case]


# ------------------------------------------------------------------------------ (a) inference forward against the float64 oracle
@pytest.mark.parametrize('ct,cc,ctrl,B,T', [
    (22, 272, True, 2, 144),       # the reference's other configuration (repr_abs_only=False)
    (22, 272, False, 3, 48),       # width 22 without the control branch
    (32, 320, True, 2, 16),        # both limits, the shortest clip, no pad column in the 32-wide rows
    (1, 1, True, 2, 32),           # the smallest widths
    (4, 100, True, 1, 48),         # the classes' default width; a control width that is no multiple of 32
    (13, 272, True, 1, 512),       # the GroupNorm limit: groups of 4096 values
    (22, 272, False, 2, 512)])
def test_forward_vs_oracle(ct, cc, ctrl, B, T):
    net, sd = make_trajnet(weight_seed(ct, ctrl), ctrl, ct, cc)
    x, c, k, t, _ = inputs(B, T, ct=ct, cc=cc)
    ref = forward64((ct, cc, ctrl, B, T), sd, x, c, k, t)
    y = net({'x_t': x.to(DEV), 'cond': c.to(DEV), 'control_cond': k.to(DEV)}, t.to(DEV)).cpu()
    e = max_abs(y, ref)
    print(f'[{ct},{cc},{ctrl},{B},{T}] forward-vs-f64 {e:.3e}  |out|max {float(ref.abs().max()):.3f}')
    assert y.shape == (B, T, ct) and e < 2e-4


# ------------------------------------------------------------------------------ (b) the sampling loop, both forms
def _loop_case(ct, cc, ctrl, B, T):
    net, sd = make_trajnet(weight_seed(ct, ctrl) + 1, ctrl, ct, cc)
    cond, k = seeded(5, B, T, ct), seeded(6, B, T, cc)
    x_T, noises = cpu_noise_sequence(8, (B, T, ct), STEPS)
    batch = {'cond': cond.to(DEV), 'control_cond': k.to(DEV)}
    fn = lambda x, i: nets.trajnet_forward(sd, x, cond, torch.full((B,), i, dtype=torch.int64), control_cond=k if ctrl else None)
    return net, batch, x_T, noises, fn


@pytest.mark.parametrize('ct,cc,ctrl,B,T', [(22, 272, True, 3, 144), (22, 272, False, 3, 144), (32, 320, True, 2, 16)])
def test_sampling_loop_both_forms(monkeypatch, ct, cc, ctrl, B, T):
    """The launch-per-layer loop (traj_tail_kernel) against the oracle's sampler driven by the oracle network, and the clip-resident
    step (its own head in tail_op) against the launch-per-layer loop, bit-identical on a repeat.  A head that served only the
    first 13 channels would pass every other loop test of the suite."""
    net, batch, x_T, noises, fn = _loop_case(ct, cc, ctrl, B, T)
    shape = (B, T, ct)
    monkeypatch.setenv('ROHM_TRAJ_RESIDENT', '0')
    y0 = _loop(net, batch, shape, x_T, noises, steps=STEPS).clone()
    assert _lib.lib().rohm_trajnet_loop_mode() == 0
    ref = odiff.p_sample_loop(fn, x_T, noises, odiff.tables(odiff.cosine_betas(STEPS)), list(range(STEPS))[::-1])
    e_o = max_abs(y0.cpu(), ref)
    monkeypatch.setenv('ROHM_TRAJ_RESIDENT', '1')
    y1 = _loop(net, batch, shape, x_T, noises, fused_chunk=4, steps=STEPS).clone()      # chunks of 4 + 4 + 2 steps: three calls
    assert _lib.lib().rohm_trajnet_loop_mode() == 1
    e_r = max_abs(y1, y0)
    print(f'[{ct},{cc},{ctrl},{B},{T}] loop-vs-oracle {e_o:.3e}  resident-vs-per-layer {e_r:.3e}')
    assert y0.shape == shape and e_o < 1e-3
    assert torch.isfinite(y1).all() and e_r < 2e-5
    assert torch.equal(y1, _loop(net, batch, shape, x_T, noises, fused_chunk=4, steps=STEPS))
    assert _lib.lib().rohm_trajnet_loop_mode() == 1


@pytest.mark.parametrize('resident', ['0', '1'])
def test_last_step_outputs_at_width_22(monkeypatch, resident):
    """x0_last (the head's own output of the last step) and x_in_last (that step's input) are written per channel by the tail of
    either loop form: both against the oracle's last step."""
    ct, cc, ctrl, B, T = 22, 272, True, 3, 144
    net, batch, x_T, noises, fn = _loop_case(ct, cc, ctrl, B, T)
    monkeypatch.setenv('ROHM_TRAJ_RESIDENT', resident)
    diff = make_diffusion(STEPS)
    diff.noise_source = lambda step, like: (x_T if step == -1 else noises[step])
    x0_last = diff.p_sample_loop(model=net, batch=batch, shape=[B, T, ct], early_stop=True)
    assert _lib.lib().rohm_trajnet_loop_mode() == int(resident)
    trace = odiff.p_sample_loop(fn, x_T, noises, odiff.tables(odiff.cosine_betas(STEPS)), list(range(STEPS))[::-1], return_all=True)
    e_x0, e_in = max_abs(x0_last.cpu(), trace[-1][1]), max_abs(batch['x_t'].cpu(), trace[-2][0])
    print(f'resident={resident} x0_last-vs-oracle {e_x0:.3e}  x_in_last-vs-oracle {e_in:.3e}')
    assert x0_last.shape == (B, T, ct) and batch['x_t'].shape == (B, T, ct)
    assert e_x0 < 1e-3 and e_in < 1e-3


# ------------------------------------------------------------------------------ (c) training gradients against float64 autograd
@pytest.mark.parametrize('ct,cc,ctrl,B,T', [
    (22, 272, True, 2, 144),
    (22, 272, False, 3, 48),
    (32, 320, True, 2, 16),
    (1, 1, True, 2, 32),
    (4, 100, True, 1, 48),
    (13, 272, False, 2, 512),      # 516 padded rows: one clip per slab, the slab longer than kSlabRows
    (13, 272, True, 3, 256),       # 260 rows: one clip per slab at level 0 (three slabs), three per slab at level 1 (one)
    (13, 272, False, 5, 160)])     # 164 rows: three clips per slab at level 0 (3 + 2), six at level 1
def test_gradients_match_float64_autograd(ct, cc, ctrl, B, T):
    net, sd = make_net(ctrl, seed=weight_seed(ct, ctrl), ct=ct, cc=cc)
    x, c, k, t, cot = inputs(B, T, ct=ct, cc=cc)
    dev = device_grads(net, x, c, k, t, cot, ctrl, ct=ct)
    ref = ref_grads(sd, x, c, k, t, cot, ctrl)
    e = max_abs(dev[0].cpu(), ref[0])
    print(f'[{ct},{cc},{ctrl},{B},{T}] train-forward-vs-f64 {e:.3e}')
    assert dev[0].shape == (B, T, ct) and e < 2e-4
    check_all(dev, ref, ctrl, f'[{ct},{cc},{ctrl},{B},{T}]', ct=ct)
    if (ct, T) == (22, 144):       # a second full run: bitwise equal
        dev2 = device_grads(net, x, c, k, t, cot, ctrl, ct=ct)
        assert torch.equal(dev[0], dev2[0]) and torch.equal(dev[2], dev2[2]) and torch.equal(dev[3], dev2[3])
        assert torch.equal(dev[4], dev2[4])
        assert all(a is None and dev2[1][n] is None if a is None else torch.equal(a, dev2[1][n]) for n, a in dev[1].items())


def test_frozen_backbone_and_input_only_at_width_22():
    """tests/test_gpu_trajnet_train.py::test_frozen_backbone_and_input_only at (22, 272): ControlNet gradients only, then the
    x_t gradient only."""
    ct, cc, ctrl, B, T = 22, 272, True, 2, 144
    net, sd = make_net(ctrl, seed=weight_seed(ct, ctrl) + 2, ct=ct, cc=cc)
    freeze_backbone(net)
    assert net.training
    x, c, k, t, cot = inputs(B, T, seed=13, ct=ct, cc=cc)
    ref = ref_grads(sd, x, c, k, t, cot, ctrl)
    net.zero_grad(set_to_none=True)
    out = net({'x_t': x.to(DEV), 'cond': c.to(DEV), 'control_cond': k.to(DEV)}, t.to(DEV))
    assert out.grad_fn is not None
    (out * cot.to(DEV)).sum().backward()
    worst = 0.0
    for n, p in net.named_parameters():
        if n.startswith('controlnet.'):
            e = rel(p.grad, ref[1][n])
            worst = max(worst, e)
            assert e <= REL_BAR, (n, e)
        else:
            assert p.grad is None, n
    for p in net.parameters():
        p.requires_grad = False
    xg = x.to(DEV).requires_grad_(True)
    net.zero_grad(set_to_none=True)
    out = net({'x_t': xg, 'cond': c.to(DEV), 'control_cond': k.to(DEV)}, t.to(DEV))
    (out * cot.to(DEV)).sum().backward()
    e_x = rel(xg.grad, ref[2])
    print(f'frozen backbone: worst controlnet gradient rel {worst:.3e}; input only: d x_t rel {e_x:.3e}')
    assert e_x <= REL_BAR, e_x
    assert all(p.grad is None for p in net.parameters())


# ------------------------------------------------------------------------------ (d) train forward = inference forward
TRAIN_EVAL_BAR = {(22, 272, True, 2, 144): 3.5e-5, (13, 272, False, 2, 512): 5.3e-5}


@pytest.mark.parametrize('ct,cc,ctrl,B,T', list(TRAIN_EVAL_BAR))
def test_train_forward_equals_inference_forward(ct, cc, ctrl, B, T):
    """Method of tests/test_gpu_trajnet_train.py::test_train_forward_equals_inference_forward (other kernels, other summation
    orders: no bitwise equality), whose bar 3.5e-5 is ten times the largest train-vs-eval difference seen at T <= 144.  Measured on
    an MI355X against the float64 oracle, max abs:
      (22, 272, ctrl, B 2, T 144), |out|max 3.0: train 2.6e-6, eval 1.5e-6, torch float32 1.4e-6, train-vs-eval 3.0e-6 -- 3.5e-5 holds;
      (13, 272, B 2, T 512), |out|max 4.6: train 4.4e-6, eval 1.6e-6, torch float32 1.9e-6, train-vs-eval 5.2e-6.
    Groups of 4096 values and larger outputs: at T = 512 the bar is that docstring's rule applied here, 10 x 5.245e-6 -> 5.3e-5."""
    net, sd = make_net(ctrl, seed=weight_seed(ct, ctrl), ct=ct, cc=cc)
    x, c, k, t, _ = inputs(B, T, ct=ct, cc=cc)
    batch = {'x_t': x.to(DEV), 'cond': c.to(DEV), 'control_cond': k.to(DEV)}
    y_train = net.train()(batch, t.to(DEV))
    assert y_train.grad_fn is not None
    with torch.no_grad():
        y_eval = net.eval()(batch, t.to(DEV))
    case = (ct, cc, ctrl, B, T)
    ref = forward64(case, sd, x, c, k, t)
    y32 = nets.trajnet_forward(sd, x, c, t, control_cond=k if ctrl else None, dtype=torch.float32)
    e_t, e_e, e_te = max_abs(y_train.detach().cpu(), ref), max_abs(y_eval.cpu(), ref), max_abs(y_train.detach(), y_eval)
    print(f'[{ct},{cc},{ctrl},{B},{T}] train-vs-f64 {e_t:.3e}  eval-vs-f64 {e_e:.3e}  torch-f32-vs-f64 {max_abs(y32, ref):.3e}  '
          f'train-vs-eval {e_te:.3e}  |out|max {float(ref.abs().max()):.3f}')
    assert e_t < 2e-4 and e_e < 2e-4
    assert e_te <= TRAIN_EVAL_BAR[case]


# ------------------------------------------------------------------------------ (e) refusals, each before any launch
def _launches(fn):
    """(the labelled launches -- convolutions, GroupNorm, the loop's tail -- a call made, the RohmHipError it raised or None)."""
    err = None
    _lib.profile_start(1)
    try:
        fn()
    except _lib.RohmHipError as e:
        err = e
    finally:
        rows = _lib.profile_stop()
    return rows, err


@pytest.mark.parametrize('ct,cc,ctrl', [(33, 272, False), (13, 321, True)])
def test_widths_past_the_limits_are_refused_at_create(ct, cc, ctrl):
    net, _ = make_trajnet(1, ctrl, ct, cc)      # the module holds parameters only: the native handle is made by the first use
    B, T = 1, 16
    batch = {'x_t': torch.zeros(B, T, ct, device=DEV), 'cond': torch.zeros(B, T, ct, device=DEV),
             'control_cond': torch.zeros(B, T, cc, device=DEV)}
    t = torch.zeros(B, dtype=torch.int64, device=DEV)
    rows, err = _launches(lambda: net(batch, t))
    assert err is not None and 'rohm_trajnet_create' in str(err) and 'bad channel counts' in str(err), err
    assert rows == {}
    tnet, _ = make_net(ctrl, seed=1, ct=ct, cc=cc)
    rows, err = _launches(lambda: tnet(batch, t))
    assert err is not None and f'traj_feat_dim={ct} control_cond_dim={cc}' in str(err), err
    assert rows == {}


@pytest.mark.parametrize('T', [528, 24])
def test_training_refuses_clip_lengths_outside_the_domain(T):
    import re
    net, _ = make_net(False, seed=1)
    x = torch.zeros(1, T, 13, device=DEV)
    rows, err = _launches(lambda: net({'x_t': x, 'cond': x}, torch.zeros(1, dtype=torch.int64, device=DEV)))
    assert err is not None and re.search(f'T={T} .*T a multiple of 16 with T <= 512', str(err)), err
    assert rows == {}


def test_inference_refuses_528_frames_before_any_launch():
    """8 channels x 528 frames is more than a GroupNorm workgroup holds (256 threads x 16 values); the forward and the sampling loop
    say so before their first convolution."""
    net, _ = make_trajnet(1, False)
    x = torch.zeros(1, 528, 13, device=DEV)
    t = torch.zeros(1, dtype=torch.int64, device=DEV)
    message = 'GroupNorm group of 8 x 528 values is not supported'
    rows, err = _launches(lambda: net({'x_t': x, 'cond': x}, t))
    assert err is not None and message in str(err), err
    assert rows == {}
    x_T, noises = cpu_noise_sequence(8, (1, 528, 13), 2)
    rows, err = _launches(lambda: _loop(net, {'cond': x}, (1, 528, 13), x_T, noises, steps=2))
    assert err is not None and message in str(err), err
    assert rows == {}
    y = net({'x_t': x[:, :512].contiguous(), 'cond': x[:, :512].contiguous()}, t)      # the handle still serves the limit itself
    assert y.shape == (1, 512, 13) and torch.isfinite(y).all()


def test_cond_dim_must_equal_traj_feat_dim():
    from rohm_amd.model.trajnet import TrajNet
    with pytest.raises(ValueError, match='cond_dim == traj_feat_dim'):
        TrajNet(time_dim=32, mid_dim=512, cond_dim=13, traj_feat_dim=22, trajcontrol=False, device=DEV)
