"""GPU: TrajNet / TrajControl's training path (rohm_trajnet_train_forward / _backward behind TrajNet.forward in train mode with
grad, and GaussianDiffusionTrajNet.training_losses) against torch autograd in float64 on the CPU through oracle.nets: all
parameter and input gradients, the reference's zero initialisation, the frozen-backbone fine-tune, bitwise reproducibility, the
differentiable loss report, short AdamW runs, the unchanged inference paths and the refused shapes."""
import types

import numpy as np
import pytest
import torch

from helpers import PoseDataset, max_abs, seeded
from oracle import geometry as G
from oracle import nets
from rohm_amd import _lib
from rohm_amd.model.trajnet import TrajNet, weight_order
from rohm_amd.utils import synth
from test_gpu_trajnet import make_diffusion

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
REL_BAR = 1e-4      # relative Frobenius error of a float32 device gradient against float64 autograd (test_gpu_posenet_train.py)
ABS_CH = [0, 2, 3, 6, 7, 8, 9, 10, 11, 12, 16, 17, 18]
UNUSED = ('cond_downsample4.conv.weight', 'cond_downsample4.conv.bias')


def make_net(ctrl, seed=0, zero_convs_random=True, ct=13, cc=272, **kw):
    """ct / cc: traj_feat_dim (= cond_dim) and control_cond_dim; the defaults are the drivers' repr_abs_only=True widths."""
    net = TrajNet(time_dim=32, mid_dim=512, cond_dim=ct, traj_feat_dim=ct, trajcontrol=ctrl, control_cond_dim=cc, device=DEV, **kw)
    sd = synth.trajnet_state_dict(seed, traj_feat_dim=ct, cond_dim=ct, trajcontrol=ctrl, control_cond_dim=cc,
                                  zero_convs_random=zero_convs_random)
    net.load_state_dict(sd, strict=True)
    return net.to(DEV).train(), sd


def inputs(B, T, seed=1, ct=13, cc=272):
    x, c, cc, cot = seeded(seed, B, T, ct), seeded(seed + 1, B, T, ct), seeded(seed + 2, B, T, cc), seeded(seed + 3, B, T, ct)
    t = torch.tensor([(37 * i + 3) % 100 for i in range(B)])      # per-sample distinct (up to B = 100)
    return x, c, cc, t, cot


def rel(a, ref):
    return float((a.detach().double().cpu() - ref.double()).norm() / ref.double().norm().clamp_min(1e-30))


def names(ctrl, ct=13):
    return weight_order(512, ct, ctrl)


def ref_grads(sd, x, c, cc, t, cot, ctrl, loss_fn=None):
    """(out, {name: grad}, dx, dc, dcc) of sum(out * cot) (or loss_fn(out)) by torch autograd on the CPU in float64."""
    sdg = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    xg, cg = x.double().clone().requires_grad_(True), c.double().clone().requires_grad_(True)
    kg = cc.double().clone().requires_grad_(True) if ctrl else None
    out = nets.trajnet_forward(sdg, xg, cg, t, control_cond=kg, dtype=torch.float64)
    ((out * cot.double()).sum() if loss_fn is None else loss_fn(out)).backward()
    return out.detach(), {k: v.grad for k, v in sdg.items()}, xg.grad, cg.grad, (kg.grad if ctrl else None)


def device_grads(net, x, c, cc, t, cot, ctrl, input_grads=True, ct=13):
    xg = x.to(DEV).requires_grad_(input_grads)
    cg = c.to(DEV).requires_grad_(input_grads)
    kg = cc.to(DEV).requires_grad_(input_grads)
    net.zero_grad(set_to_none=True)
    out = net({'x_t': xg, 'cond': cg, 'control_cond': kg}, t.to(DEV))
    assert out.grad_fn is not None
    (out * cot.to(DEV)).sum().backward()
    named = dict(net.named_parameters())
    return out.detach(), {k: named[k].grad for k in names(ctrl, ct)}, xg.grad, cg.grad, (kg.grad if ctrl else None)


def check_all(dev, ref, ctrl, label='', ct=13):
    _, g, dx, dc, dk = dev
    _, g64, dx64, dc64, dk64 = ref
    worst = ('', 0.0)
    for k in names(ctrl, ct):
        if k in UNUSED:
            assert g[k] is None and g64[k] is None, k
            continue
        e = rel(g[k], g64[k])
        print(f'{label} {k}: rel {e:.3e}  |g64| {float(g64[k].norm()):.3e}')
        worst = max(worst, (k, e), key=lambda z: z[1])
        assert e <= REL_BAR, (k, e)
    pairs = [('d x_t', dx, dx64), ('d cond', dc, dc64)] + ([('d control_cond', dk, dk64)] if ctrl else [])
    for name, a, r in pairs:
        e = rel(a, r)
        print(f'{label} {name}: rel {e:.3e}')
        assert e <= REL_BAR, (name, e)
    print(f'{label} worst parameter {worst}')
    return worst


# ------------------------------------------------------------------------------ 1. gradients against float64 autograd
@pytest.mark.parametrize('ctrl,B,T', [(False, 1, 144), (False, 3, 144), (True, 3, 144), (True, 2, 48), (False, 5, 16),
                                      (True, 32, 144), (False, 64, 144)])
def test_gradients_match_float64_autograd(ctrl, B, T):
    net, sd = make_net(ctrl, seed=40 + B)
    x, c, cc, t, cot = inputs(B, T)
    dev = device_grads(net, x, c, cc, t, cot, ctrl)
    ref = ref_grads(sd, x, c, cc, t, cot, ctrl)
    assert max_abs(dev[0].cpu(), ref[0]) < 2e-4
    check_all(dev, ref, ctrl, f'[{ctrl},{B},{T}]')


# ------------------------------------------------------------------------------ 2. train forward = inference forward
@pytest.mark.parametrize('ctrl,B,T', [(False, 3, 144), (True, 3, 144), (True, 32, 144), (False, 5, 16)])
def test_train_forward_equals_inference_forward(ctrl, B, T):
    """Train mode with grad and eval mode under no_grad compute the same function with different kernels (other tile shapes and
    summation orders, GroupNorm statistics in another order), so bitwise equality is not demanded.  Measured on an MI355X over
    these four cases, outputs of magnitude up to ~3: max |train - eval| 2.1e-6 ... 3.5e-6, the train forward 1.9e-6 ... 3.1e-6 and
    the inference forward 1.2e-6 ... 2.4e-6 from the float64 oracle -- about 1e-6 relative, the size of the 5.6e-7 relative error
    torch's float32 forward shows.  The bar is 10x the largest difference observed."""
    net, sd = make_net(ctrl, seed=7)
    x, c, cc, t, _ = inputs(B, T, seed=5)
    batch = {'x_t': x.to(DEV), 'cond': c.to(DEV), 'control_cond': cc.to(DEV)}
    y_train = net.train()(batch, t.to(DEV))
    assert y_train.grad_fn is not None
    with torch.no_grad():
        y_eval = net.eval()(batch, t.to(DEV))
    ref = nets.trajnet_forward(sd, x, c, t, control_cond=cc if ctrl else None, dtype=torch.float64)
    e_t, e_e, e_te = max_abs(y_train.detach().cpu(), ref), max_abs(y_eval.cpu(), ref), max_abs(y_train.detach(), y_eval)
    print(f'train-vs-f64 {e_t:.3e}  eval-vs-f64 {e_e:.3e}  train-vs-eval {e_te:.3e}  |out|max {float(ref.abs().max()):.3f}')
    assert e_t < 2e-4 and e_e < 2e-4
    assert e_te <= 3.5e-5


# ------------------------------------------------------------------------------ 3. the reference's zero initialisation
def test_zero_initialised_control_convs():
    ctrl, B, T = True, 2, 144
    net, sd = make_net(ctrl, seed=5, zero_convs_random=False)
    x, c, cc, t, cot = inputs(B, T, seed=9)
    _, g, dx, dc, dk = device_grads(net, x, c, cc, t, cot, ctrl)
    _, g64, dx64, dc64, dk64 = ref_grads(sd, x, c, cc, t, cot, ctrl)
    n_zero = 0
    for k in names(ctrl):
        if k in UNUSED:
            assert g[k] is None
            continue
        if k.startswith('controlnet.') and int(torch.count_nonzero(g64[k])) == 0:
            n_zero += 1
            assert int(torch.count_nonzero(g[k])) == 0 and not torch.isnan(g[k]).any(), k
        else:
            assert rel(g[k], g64[k]) <= REL_BAR, (k, rel(g[k], g64[k]))
    # the 72 parameters upstream of zero convs 1..4 / mid, and zero conv 0's own two (its output only reaches the loss through them)
    assert n_zero == 74
    for k in [k for k in names(ctrl) if 'control_zero_conv_' in k and not k.startswith('controlnet.control_zero_conv_0')]:
        assert float(g64[k].norm()) > 0, k      # the zero convs downstream of a live input learn from the first step
    assert int(torch.count_nonzero(dk)) == 0 and int(torch.count_nonzero(dk64)) == 0
    assert rel(dx, dx64) <= REL_BAR and rel(dc, dc64) <= REL_BAR


# ------------------------------------------------------------------------------ 4. frozen backbone
def freeze_backbone(net):
    """train_trajnet.py:166-175."""
    for name, param in net.named_parameters():
        param.requires_grad = name.split('.')[0].split('_')[0] == 'controlnet'
    for name, layer in net.named_modules():
        if name.split('.')[0].split('_')[0] in ['cond', 'diff', 'time']:
            layer.eval()


def test_frozen_backbone_and_input_only():
    ctrl, B, T = True, 3, 144
    net, sd = make_net(ctrl, seed=21)
    freeze_backbone(net)
    assert net.training
    x, c, cc, t, cot = inputs(B, T, seed=13)
    ref = ref_grads(sd, x, c, cc, t, cot, ctrl)
    net.zero_grad(set_to_none=True)
    out = net({'x_t': x.to(DEV), 'cond': c.to(DEV), 'control_cond': cc.to(DEV)}, t.to(DEV))
    assert out.grad_fn is not None
    (out * cot.to(DEV)).sum().backward()
    frozen_gemms = _lib.lib().rohm_trajnet_train_last_gemms()
    for k, p in net.named_parameters():
        if k.startswith('controlnet.'):
            e = rel(p.grad, ref[1][k])
            assert e <= REL_BAR, (k, e)
        else:
            assert p.grad is None, k
    # everything trainable launches more GEMMs than the fine-tune step
    for p in net.parameters():
        p.requires_grad = True
    device_grads(net, x, c, cc, t, cot, ctrl, input_grads=False)
    all_gemms = _lib.lib().rohm_trajnet_train_last_gemms()
    print(f'GEMM launches of the backward: frozen backbone {frozen_gemms}, all trainable {all_gemms}')
    assert 0 < frozen_gemms < all_gemms
    # all parameters frozen, only x_t wants a gradient
    for p in net.parameters():
        p.requires_grad = False
    xg = x.to(DEV).requires_grad_(True)
    net.zero_grad(set_to_none=True)
    out = net({'x_t': xg, 'cond': c.to(DEV), 'control_cond': cc.to(DEV)}, t.to(DEV))
    (out * cot.to(DEV)).sum().backward()
    assert rel(xg.grad, ref[2]) <= REL_BAR, rel(xg.grad, ref[2])
    assert all(p.grad is None for p in net.parameters())


# ------------------------------------------------------------------------------ 5. bitwise reproducibility
def test_gradients_are_bitwise_reproducible():
    ctrl, B, T = True, 32, 144
    net, _ = make_net(ctrl, seed=3)
    x, c, cc, t, cot = inputs(B, T, seed=17)
    params = net.train_parameters()
    live = [p for k, p in zip(names(ctrl), params) if k not in UNUSED]

    def forward():
        return net({'x_t': x.to(DEV), 'cond': c.to(DEV), 'control_cond': cc.to(DEV)}, t.to(DEV))
    out = forward()
    loss = (out * cot.to(DEV)).sum()
    g1 = torch.autograd.grad(loss, live, retain_graph=True)
    g2 = torch.autograd.grad(loss, live, retain_graph=True)      # the same saved forward
    out3 = forward()
    g3 = torch.autograd.grad((out3 * cot.to(DEV)).sum(), live)   # a full second run
    assert torch.equal(out, out3)
    for a, b, d in zip(g1, g2, g3):
        assert torch.equal(a, b) and torch.equal(a, d)


# ------------------------------------------------------------------------------ 6. the loss and training_losses
STAGE1 = dict(weight_loss_root_rec_repr=1.0, weight_loss_root_pos_global=100.0, weight_loss_root_vel_global=1000.0,
              weight_loss_root_rot_vel_from_abs_traj=1.0, weight_loss_root_smplx_transl_vel=1000.0,
              weight_loss_root_smplx_rot_vel=1.0, weight_loss_root_smooth=1.0,
              weight_loss_root_rot_cos_smooth_from_abs_traj=1.0)      # cfg_files/train_cfg/trajnet_train_vanilla_stage1.yaml


def _loss64(w, mean, std, clean, out, body64):
    """float64 restatement of model/trajnet.py:277-400 with repr_abs_only=True (`loss` only); clean [B,T,294] normalised,
    out [B,T,13]."""
    mean, std = torch.from_numpy(mean).double(), torch.from_numpy(std).double()
    cols = [clean[..., i:i + 1] for i in range(clean.shape[-1])]
    for j, ch in enumerate(ABS_CH):
        cols[ch] = out[..., j:j + 1]
    rec = torch.cat(cols, dim=-1)
    sq = (clean - rec) ** 2
    l_repr = sq[..., ABS_CH].mean()
    fc, fr = clean * std + mean, rec * std + mean
    dc, dr = G.split_repr(fc), G.split_repr(fr)
    root_clean = G.joints_from_abs_traj(dc)[:, :, 0]
    roots = [G.joints_from_abs_traj(dr)[:, :, 0], G.joints_from_smplx(dr, body64, through_axis_angle=False)[:, :, 0]]
    diff = lambda x: x[:, 1:] - x[:, :-1]
    pos = sum(((r - root_clean) ** 2).mean() for r in roots)      # the rel_traj terms are set to 0 (trajnet.py:386-389)
    vel = sum(((diff(r) - diff(root_clean)) ** 2).mean() for r in roots)
    smooth = sum((diff(diff(r)) ** 2).mean() for r in roots)
    bs = clean.shape[0]
    R = G.rot6d_to_rotmat(dr['smplx_rot_6d'].reshape(-1, 6)).reshape(bs, -1, 3, 3)
    wv = torch.matmul(R[:, 1:] - R[:, :-1], R[:, :-1].transpose(-1, -2))
    rot_vel = torch.stack([(-wv[..., 1, 2] + wv[..., 2, 1]) / 2.0, (wv[..., 0, 2] - wv[..., 2, 0]) / 2.0,
                           (-wv[..., 0, 1] + wv[..., 1, 0]) / 2.0], dim=-1)
    l_rot_vel = ((rot_vel - dc['smplx_rot_vel'][:, :-1]) ** 2).mean()
    l_transl_vel = ((diff(dr['smplx_trans']) - dc['smplx_trans_vel'][:, :-1]) ** 2).mean()
    cos_vel = lambda d: torch.cos(d['root_rot_angle'][:, 1:] * 2) - torch.cos(d['root_rot_angle'][:, :-1] * 2)
    cv = cos_vel(dr)
    l_cos_vel = ((cos_vel(dc) - cv) ** 2).mean()
    l_cos_smooth = (diff(cv) ** 2).mean()
    return (w['weight_loss_root_rec_repr'] * l_repr + w['weight_loss_root_pos_global'] * pos +
            w['weight_loss_root_vel_global'] * vel + w['weight_loss_root_rot_vel_from_abs_traj'] * l_cos_vel +
            w['weight_loss_root_smplx_transl_vel'] * l_transl_vel + w['weight_loss_root_smplx_rot_vel'] * l_rot_vel +
            w['weight_loss_root_smooth'] * smooth + w['weight_loss_root_rot_cos_smooth_from_abs_traj'] * l_cos_smooth)


@pytest.fixture(scope='module')
def body():
    from rohm_amd.body_model import SMPLXLayer
    bt = synth.synthetic_smplx_tensors(0)
    return SMPLXLayer.from_tensors(bt).to(DEV), G.BodyModel(bt, dtype=torch.float64)


def _clean(seed, B, T, mean, std):
    return synth.plausible_motion(seed, B, T, mean, std)[:, :, 0].permute(0, 2, 1).contiguous()      # [B, T, 294]


def test_loss_backpropagates_into_model_output(body):
    from rohm_amd.model.eval_losses import trajnet_losses
    layer, body64 = body
    mean, std = synth.synthetic_stats(0)
    net = types.SimpleNamespace(dataset=PoseDataset(mean, std), repr_abs_only=True, traj_feat_dim=13, **STAGE1)
    B, T = 2, 144
    clean = _clean(11, B, T, mean, std)
    out0 = clean[..., ABS_CH] + 0.05 * seeded(12, B, T, 13)
    out = out0.to(DEV).requires_grad_(True)
    d = trajnet_losses(net, {'motion_repr_clean': clean.to(DEV)}, out, layer)
    d['loss'].backward()
    d0 = trajnet_losses(net, {'motion_repr_clean': clean.to(DEV)}, out0.to(DEV), layer)
    for k in d0:
        assert torch.equal(d[k].detach(), d0[k]), k
    out64 = out0.double().requires_grad_(True)
    loss64 = _loss64(STAGE1, mean, std, clean.double(), out64, body64)
    loss64.backward()
    assert abs(float(d['loss'].detach()) - float(loss64.detach())) <= 1e-4 * abs(float(loss64.detach()))
    e = rel(out.grad, out64.grad)
    print(f'd loss / d model_output: rel {e:.3e}')
    assert e <= REL_BAR, e


def test_training_losses_is_the_references(body):
    layer, body64 = body
    mean, std = synth.synthetic_stats(0)
    net, sd = make_net(False, seed=2, dataset=PoseDataset(mean, std), repr_abs_only=True, **STAGE1)
    diff = make_diffusion()
    B, T = 4, 144
    g = torch.Generator().manual_seed(11)
    clean = _clean(11, B, T, mean, std).to(DEV)
    cond = (clean[..., :13] + 0.1 * torch.randn(B, T, 13, generator=g).to(DEV)).contiguous()
    noise = torch.randn(B, T, 13, generator=g).to(DEV)
    t = torch.randint(0, 100, (B,), generator=g).to(DEV)
    batch = {'motion_repr_clean': clean, 'cond': cond}
    loss_dict = diff.training_losses(net, batch, t, noise=noise, traj_feat_dim=13, smplx_model=layer)
    assert isinstance(loss_dict, dict) and loss_dict['loss'].requires_grad
    a = torch.from_numpy(diff.sqrt_alphas_cumprod).float().to(DEV)[t][:, None, None]
    b = torch.from_numpy(diff.sqrt_one_minus_alphas_cumprod).float().to(DEV)[t][:, None, None]
    assert float((batch['x_t'] - (a * clean[..., :13] + b * noise)).abs().max()) <= 1e-6
    net.zero_grad(set_to_none=True)
    loss_dict['loss'].backward()
    with torch.no_grad():
        ref = net.eval().compute_losses_with_smpl(batch, net(batch, t), layer)
    net.train()
    for k in ref:
        assert torch.allclose(loss_dict[k].detach(), ref[k], rtol=1e-5, atol=1e-7), (k, float(loss_dict[k]), float(ref[k]))
    # the wrapped model is accepted like the plain module
    wrapped = diff._wrap_model(net) if hasattr(diff, '_wrap_model') else types.SimpleNamespace(model=net)
    again = diff.training_losses(wrapped, dict(batch), t, noise=noise, traj_feat_dim=13, smplx_model=layer)
    assert torch.equal(again['loss'].detach(), loss_dict['loss'].detach())
    # every parameter gradient against the float64 chain (oracle forward + the restated loss); where torch's own float32
    # autograd of that chain misses the bar as well, the bound is 4x torch's error
    xt, cd, tc = batch['x_t'].cpu(), cond.cpu(), t.cpu()
    loss_fn = lambda o: _loss64(STAGE1, mean, std, clean.cpu().double(), o, body64)
    _, g64, _, _, _ = ref_grads(sd, xt, cd, None, tc, None, False, loss_fn=loss_fn)
    g32 = None
    named = dict(net.named_parameters())
    needed = []
    for k in names(False):
        if k in UNUSED:
            assert named[k].grad is None
            continue
        e = rel(named[k].grad, g64[k])
        bar = REL_BAR
        if e > REL_BAR:
            if g32 is None:
                g32 = _torch32_loss_grads(sd, xt, cd, tc, clean, mean, std, layer, net)
            e32 = rel(g32[k], g64[k])
            bar = max(REL_BAR, 4 * e32)
            needed.append((k, e, e32))
        assert e <= bar, (k, e, bar)
    print('parameters that needed the torch-float32 bound:', needed)


def _torch32_loss_grads(sd, xt, cd, tc, clean, mean, std, layer, net):
    """torch's float32 autograd of the same chain on the GPU: oracle forward in float32 + the device loss report."""
    sdg = {k: v.to(DEV).requires_grad_(True) for k, v in sd.items()}
    with torch.device(DEV):      # the oracle builds its frequency table with a default-device factory call
        o = nets.trajnet_forward(sdg, xt.to(DEV), cd.to(DEV), tc.to(DEV))
    net.compute_losses_with_smpl({'motion_repr_clean': clean}, o, layer)['loss'].backward()
    return {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in sdg.items()}


# ------------------------------------------------------------------------------ 7. training runs
def _fit(net, diff, batch, t, noise, layer, steps=30):
    opt = torch.optim.AdamW([p for p in net.parameters() if p.requires_grad], lr=1e-4)
    losses = []
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        d = diff.training_losses(net, batch, t, noise=noise, traj_feat_dim=13, smplx_model=layer)
        d['loss'].backward()
        opt.step()
        losses.append(float(d['loss'].detach()))
    return losses


@pytest.mark.parametrize('finetune', [False, True])
def test_adamw_steps_lower_the_loss(body, finetune):
    layer, _ = body
    mean, std = synth.synthetic_stats(0)
    net, sd = make_net(finetune, seed=4, zero_convs_random=not finetune, dataset=PoseDataset(mean, std), repr_abs_only=True,
                       **STAGE1)
    if finetune:
        freeze_backbone(net)
    diff = make_diffusion()
    B, T = 8, 144
    g = torch.Generator().manual_seed(5)
    clean = _clean(21, B, T, mean, std).to(DEV)
    batch = {'motion_repr_clean': clean, 'cond': (clean[..., :13] + 0.1 * torch.randn(B, T, 13, generator=g).to(DEV)).contiguous(),
             'control_cond': clean[..., 22:].contiguous()}
    noise = torch.randn(B, T, 13, generator=g).to(DEV)
    t = torch.randint(0, 100, (B,), generator=g).to(DEV)
    losses = _fit(net, diff, batch, t, noise, layer)
    print('losses', losses[0], losses[-1])
    assert losses[-1] < losses[0]
    new_sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    if finetune:
        for k, v in new_sd.items():
            if not k.startswith('controlnet.'):
                assert torch.equal(v, sd[k]), k
            elif 'control_zero_conv_' in k and k.endswith('.weight'):
                assert float(v.abs().max()) > 0, k
    # the inference path sees the updated weights
    x, c, cc, tt, _ = inputs(2, 144, seed=31)
    with torch.no_grad():
        y = net.eval()({'x_t': x.to(DEV), 'cond': c.to(DEV), 'control_cond': cc.to(DEV)}, tt.to(DEV)).cpu()
    ref = nets.trajnet_forward(new_sd, x, c, tt, control_cond=cc if finetune else None, dtype=torch.float64)
    assert max_abs(y, ref) < 2e-4
    assert max_abs(ref, nets.trajnet_forward(sd, x, c, tt, control_cond=cc if finetune else None, dtype=torch.float64)) > 1e-5


# ------------------------------------------------------------------------------ 8. unchanged paths and refusals
def test_unchanged_paths_and_refusals(monkeypatch):
    from rohm_amd.model import trajnet as tn
    net, _ = make_net(True, seed=6)
    x, c, cc, t, _ = inputs(2, 144, seed=3)
    batch = {'x_t': x.to(DEV), 'cond': c.to(DEV), 'control_cond': cc.to(DEV)}
    with torch.no_grad():
        y_eval = net.eval()(batch, t.to(DEV))

    def boom(*a, **k):
        raise AssertionError('the training path must not be taken')
    monkeypatch.setattr(tn._TrajNetTrain, 'apply', boom)
    with torch.no_grad():
        y_train_nograd = net.train()(batch, t.to(DEV))
    y_eval_grad = net.eval()(batch, t.to(DEV))
    assert y_train_nograd.grad_fn is None and y_eval_grad.grad_fn is None
    assert torch.equal(y_train_nograd, y_eval) and torch.equal(y_eval_grad, y_eval)
    monkeypatch.undo()
    net.train()
    long = {'x_t': seeded(1, 1, 150, 13).to(DEV), 'cond': seeded(2, 1, 150, 13).to(DEV), 'control_cond': seeded(3, 1, 150, 272).to(DEV)}
    with pytest.raises(_lib.RohmHipError, match='T'):
        net(long, torch.tensor([5], device=DEV))
    small = TrajNet(time_dim=32, mid_dim=256, cond_dim=13, traj_feat_dim=13, trajcontrol=False, device=DEV).to(DEV).train()
    with pytest.raises(_lib.RohmHipError, match='mid_dim'):
        small({'x_t': x.to(DEV), 'cond': c.to(DEV)}, t.to(DEV))
    with pytest.raises(KeyError):
        net({'x_t': x.to(DEV), 'cond': c.to(DEV)}, t.to(DEV))
