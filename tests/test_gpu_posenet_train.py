"""GPU: PoseNet's training path (rohm_posenet_train_forward / _backward behind PoseNet.forward in train mode with grad, and
GaussianDiffusionPoseNet.training_losses) against torch autograd in float64 through oracle.nets, with and without the five
dropouts (their masks fetched from rohm_posenet_dropout_mask); determinism, the unchanged inference paths, refused shapes."""
import math

import numpy as np
import pytest
import torch

from helpers import golden
from oracle import nets
from rohm_amd import _lib
from rohm_amd.model.posenet import PoseNet, dropout_mask, train_param_names
from rohm_amd.utils import synth

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
REL_BAR = 1e-4      # relative Frobenius error of a float32 device gradient against float64 autograd


class DS:
    pose_feat_dim, traj_feat_dim = 272, 22


def make_net(L, seed=0, dropout=0.0):
    net = PoseNet(DS(), 294, latent_dim=512, ff_size=1024, num_layers=L, num_heads=4, dropout=dropout, traj_feat_dim=22,
                  body_model_path=torch.nn.Identity(), device=DEV)
    sd = synth.posenet_state_dict(seed, num_layers=L)
    net.load_state_dict(sd, strict=True)
    return net.to(DEV).train(), sd


def inputs(B, T, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 294, 1, T, generator=g)
    c = torch.randn(B, 294, 1, T, generator=g)
    t = torch.randint(0, 1000, (B,), generator=g)
    cot = torch.randn(B, 294, 1, T, generator=g)
    return x, c, t, cot


def rel(a, ref):
    return float((a.double() - ref).norm() / ref.norm().clamp_min(1e-30))


def ref_grads(sd, x, c, t, cot, dtype, masks=None, p=0.0):
    """(out, {name: grad}, dx, dc) of sum(out * cot) by torch autograd on the CPU in `dtype`."""
    sdg = {k: (v.to(dtype).clone().requires_grad_(not k.endswith('.pe')) if v.is_floating_point() else v)
           for k, v in sd.items()}
    xg, cg = x.to(dtype).clone().requires_grad_(True), c.to(dtype).clone().requires_grad_(True)
    if masks is None:
        out = nets.posenet_forward(sdg, xg, cg, t, dtype=dtype)
    else:
        out = forward_masked(sdg, xg, cg, t, masks, p)
    (out * cot.to(dtype)).sum().backward()
    return out.detach(), {k: v.grad for k, v in sdg.items() if v.is_floating_point() and v.requires_grad}, xg.grad, cg.grad


def forward_masked(sd, x_t, cond, t, masks, p, n_head=4, traj=22):
    """oracle.nets.posenet_forward with the training path's dropout masks multiplied in (keep / (1 - p))."""
    k = 1.0 / (1.0 - p)
    dt = x_t.dtype
    m = {key: v.to(dt) * k for key, v in masks.items()}
    B, C, _, T = x_t.shape
    L = 1 + max(int(q.split('.')[2]) for q in sd if q.startswith('seqTransEncoder.layers.'))
    emb = nets.timestep_token(sd, t)
    xs, cs = x_t[:, :, 0].permute(0, 2, 1), cond[:, :, 0].permute(0, 2, 1)
    h = (xs @ sd['input_process.poseEmbedding.weight'].T + sd['input_process.poseEmbedding.bias']
         + cs @ sd['input_process_cond.poseEmbedding.weight'].T + sd['input_process_cond.poseEmbedding.bias'])
    seq = torch.cat([emb[:, None], h], dim=1) + sd['sequence_pos_encoder.pe'][:T + 1, 0][None]
    seq = seq * m[(0, 0)]
    for i in range(L):
        pre = f'seqTransEncoder.layers.{i}.'
        S, D = seq.shape[1], seq.shape[2]
        dh = D // n_head
        qkv = seq @ sd[pre + 'self_attn.in_proj_weight'].T + sd[pre + 'self_attn.in_proj_bias']
        q, kk, v = [z.view(B, S, n_head, dh).transpose(1, 2) for z in qkv.split(D, dim=-1)]
        a = torch.softmax((q @ kk.transpose(-1, -2)) / math.sqrt(dh), dim=-1) * m[(i, 1)]
        a = (a @ v).transpose(1, 2).reshape(B, S, D)
        a = (a @ sd[pre + 'self_attn.out_proj.weight'].T + sd[pre + 'self_attn.out_proj.bias']) * m[(i, 2)]
        y = nets.layer_norm(seq + a, sd[pre + 'norm1.weight'], sd[pre + 'norm1.bias'])
        f = nets.gelu_erf(y @ sd[pre + 'linear1.weight'].T + sd[pre + 'linear1.bias']) * m[(i, 3)]
        f = (f @ sd[pre + 'linear2.weight'].T + sd[pre + 'linear2.bias']) * m[(i, 4)]
        seq = nets.layer_norm(y + f, sd[pre + 'norm2.weight'], sd[pre + 'norm2.bias'])
    out = seq[:, 1:] @ sd['output_process.poseFinal.weight'].T + sd['output_process.poseFinal.bias']
    return torch.cat([cond[:, :traj], out.permute(0, 2, 1)[:, :, None]], dim=1)


def fetch_masks(seed, L, B, T, p):
    S = T + 1
    shapes = {1: (B, 4, S, S), 2: (B, S, 512), 3: (B, S, 1024), 4: (B, S, 512)}
    masks = {(0, 0): dropout_mask(seed, 0, 0, (B, S, 512), p, DEV).cpu()}
    for i in range(L):
        for site, shp in shapes.items():
            masks[(i, site)] = dropout_mask(seed, i, site, shp, p, DEV).cpu()
    return masks


def device_grads(net, x, c, t, cot):
    xg = x.detach().to(DEV).requires_grad_(True)
    cg = c.detach().to(DEV).requires_grad_(True)
    net.zero_grad(set_to_none=True)
    out = net({'x_t': xg, 'cond': cg}, t.to(DEV))
    assert out.grad_fn is not None
    (out * cot.to(DEV)).sum().backward()
    named = dict(net.named_parameters())
    return out.detach().cpu(), {k: named[k].grad.cpu() for k in train_param_names(net.num_layers)}, xg.grad.cpu(), cg.grad.cpu()


def check_against(dev, r64, r32):
    out, g, dx, dc = dev
    o64, g64, dx64, dc64 = r64
    o32, g32, dx32, dc32 = r32
    worst = {}
    for k in g:
        e, e32 = rel(g[k], g64[k]), rel(g32[k], g64[k])
        worst[k] = (e, e32)
        assert e <= REL_BAR and e <= max(8 * e32, 1e-6), (k, e, e32)
    for name, a, r, r32_ in (('d x_t', dx, dx64, dx32), ('d cond', dc, dc64, dc32)):
        e, e32 = rel(a, r), rel(r32_, r)
        assert e <= REL_BAR and e <= max(8 * e32, 1e-6), (name, e, e32)
    assert rel(out, o64) <= REL_BAR
    return worst


@pytest.mark.parametrize('L,B,T', [(2, 1, 143), (2, 3, 143), (2, 32, 143), (8, 3, 143), (2, 3, 63)])
def test_gradients_match_float64_autograd(L, B, T):
    net, sd = make_net(L)
    x, c, t, cot = inputs(B, T)
    dev = device_grads(net, x, c, t, cot)
    assert set(dev[1]) == {k for k in sd if not k.endswith('.pe')}      # pe is a buffer (held twice in the state dict)
    check_against(dev, ref_grads(sd, x, c, t, cot, torch.float64), ref_grads(sd, x, c, t, cot, torch.float32))


def test_dropout_matches_masked_float64_and_reproduces():
    L, B, T, p = 2, 2, 63, 0.1
    net, sd = make_net(L, dropout=p)
    x, c, t, cot = inputs(B, T, seed=5)
    torch.manual_seed(123)
    dev = device_grads(net, x, c, t, cot)
    seed = net.last_dropout_seed
    masks = fetch_masks(seed, L, B, T, p)
    check_against(dev, ref_grads(sd, x, c, t, cot, torch.float64, masks, p), ref_grads(sd, x, c, t, cot, torch.float32, masks, p))
    # keep fraction of every site within 5 sigma of 1 - p
    for key, mk in masks.items():
        n = mk.numel()
        frac = mk.double().mean().item()
        assert abs(frac - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / n), (key, frac)
    # torch.manual_seed reproduces the step bitwise; the next call draws other masks
    torch.manual_seed(123)
    dev2 = device_grads(net, x, c, t, cot)
    assert net.last_dropout_seed == seed
    assert torch.equal(dev[0], dev2[0]) and all(torch.equal(dev[1][k], dev2[1][k]) for k in dev[1])
    device_grads(net, x, c, t, cot)
    assert net.last_dropout_seed != seed
    m2 = dropout_mask(net.last_dropout_seed, 1, 3, (B, T + 1, 1024), p, DEV).cpu()
    assert not torch.equal(m2, masks[(1, 3)])


def test_train_forward_equals_inference_forward():
    net, sd = make_net(8)
    x, c, t, _ = inputs(4, 143, seed=7)
    batch = {'x_t': x.to(DEV), 'cond': c.to(DEV)}
    out_train = net(batch, t.to(DEV))
    assert out_train.grad_fn is not None
    with torch.no_grad():
        out_eval = net.eval()(batch, t.to(DEV))
    assert float((out_train.detach() - out_eval).abs().max()) <= 1e-5
    # the committed golden at its own bar (tests/test_gpu_posenet.py)
    from helpers import seeded
    gd = golden('posenet_forward.npz')
    netg, _ = make_net(8, seed=int(gd['weight_seed']))
    xg, cg = seeded(int(gd['x_seed']), 2, 294, 1, 143), seeded(int(gd['cond_seed']), 2, 294, 1, 143)
    y = netg({'x_t': xg.to(DEV), 'cond': cg.to(DEV)}, torch.from_numpy(gd['t']).to(DEV))
    assert y.grad_fn is not None
    assert float((y.detach().cpu() - torch.from_numpy(gd['y'])).abs().max()) < 1e-4


def test_backward_is_bitwise_reproducible():
    net, _ = make_net(2)
    x, c, t, cot = inputs(3, 143, seed=9)
    out = net({'x_t': x.to(DEV), 'cond': c.to(DEV).requires_grad_(True)}, t.to(DEV))
    g1 = torch.autograd.grad(out, list(net.train_parameters()), cot.to(DEV), retain_graph=True)
    g2 = torch.autograd.grad(out, list(net.train_parameters()), cot.to(DEV))
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))


def _diffusion():
    from rohm_amd.diffusion import gaussian_diffusion_posenet as gdp
    from rohm_amd.diffusion.respace import SpacedDiffusionPoseNet
    from rohm_amd.utils.model_util import create_gaussian_diffusion

    class Args:
        noise_schedule, sigma_small = 'cosine', True
    return create_gaussian_diffusion(Args, gdp, SpacedDiffusionPoseNet, 1000, '', device=DEV)


def test_training_losses_and_adamw_steps():
    from helpers import PoseDataset
    from oracle import geometry as G
    from rohm_amd.body_model import SMPLXLayer
    from test_gpu_repr_joints_vjp import _posenet_loss64
    bt = synth.synthetic_smplx_tensors(0)
    layer, body64 = SMPLXLayer.from_tensors(bt).to(DEV), G.BodyModel(bt, dtype=torch.float64)
    mean, std = synth.synthetic_stats(0)
    L = 2
    net = PoseNet(PoseDataset(mean, std), 294, latent_dim=512, ff_size=1024, num_layers=L, num_heads=4, dropout=0.0,
                  traj_feat_dim=22, body_model_path=layer, device=DEV,
                  # the stage-1 loss weights (cfg_files/train_cfg/posenet_train_stage1.yaml)
                  weight_loss_rec_repr_full_body=1.0, weight_loss_repr_foot_contact_mse=1.0, weight_loss_joint_pos_global=100.0,
                  weight_loss_joint_vel_global=1000.0, weight_loss_joint_smooth=0.0, weight_loss_foot_skating=0.1,
                  start_skating_loss_epoch=0)
    sd = synth.posenet_state_dict(0, num_layers=L)
    net.load_state_dict(sd, strict=False)
    net = net.to(DEV).train()
    diff = _diffusion()
    B, T = 8, 143
    g = torch.Generator().manual_seed(11)
    clean = synth.plausible_motion(11, B, T, mean, std).to(DEV)
    cond = (clean + 0.1 * torch.randn(clean.shape, generator=g).to(DEV)).contiguous()
    noise = torch.randn(clean.shape, generator=g).to(DEV)
    t = torch.randint(0, 1000, (B,), generator=g).to(DEV)
    # q_sample on the device is the reference's formula
    xt = diff.q_sample(clean, t, noise)
    a = torch.from_numpy(diff.sqrt_alphas_cumprod).float().to(DEV)[t][:, None, None, None]
    b = torch.from_numpy(diff.sqrt_one_minus_alphas_cumprod).float().to(DEV)[t][:, None, None, None]
    assert float((xt - (a * clean + b * noise)).abs().max()) <= 1e-6
    batch = {'motion_repr_clean': clean, 'cond': cond}
    loss_dict, out = diff.training_losses(net, batch, t, noise=noise, epoch=0)
    assert out.grad_fn is not None and loss_dict['loss'].requires_grad
    with torch.no_grad():
        ref = net.compute_losses_with_smpl(batch, net(batch, t), epoch=0)
    for k in ref:
        assert torch.allclose(loss_dict[k].detach(), ref[k], rtol=1e-5, atol=1e-7), k
    # every parameter gradient against the float64 chain: oracle forward + the float64 loss restatement
    net.zero_grad(set_to_none=True)
    loss_dict['loss'].backward()
    sdg = {k: v.double().clone().requires_grad_(not k.endswith('.pe')) for k, v in sd.items()}
    o64 = nets.posenet_forward(sdg, xt.cpu().double(), cond.cpu().double(), t.cpu(), dtype=torch.float64)
    loss64 = _posenet_loss64(net, clean.cpu().double(), o64, body64)
    loss64.backward()
    named = dict(net.named_parameters())
    for k in train_param_names(L):
        e = rel(named[k].grad.cpu(), sdg[k].grad)
        assert e <= REL_BAR, (k, e)
    # 30 AdamW steps on the fixed batch lower the loss; the inference path then sees the new weights
    opt = torch.optim.AdamW([named[k] for k in train_param_names(L)], lr=1e-4)
    first = None
    for _ in range(30):
        opt.zero_grad(set_to_none=True)
        ld, _ = diff.training_losses(net, batch, t, noise=noise)
        ld['loss'].backward()
        opt.step()
        first = float(ld['loss'].detach()) if first is None else first
    net.eval()
    with torch.no_grad():
        last = float(diff.training_losses(net, batch, t, noise=noise)[0]['loss'])
        y_eval = net(dict(batch, x_t=xt), t)
    assert last < first
    sd_now = {k: v.detach().cpu() for k, v in net.state_dict().items() if not k.startswith('smplx_model.')}
    y_ref = nets.posenet_forward(sd_now, xt.cpu(), cond.cpu(), t.cpu())
    assert float((y_eval.cpu() - y_ref).abs().max()) < 1e-4


def test_unchanged_paths_and_refusals(monkeypatch):
    from rohm_amd.model import posenet as pn
    net, _ = make_net(2, dropout=0.1)
    x, c, t, _ = inputs(2, 143, seed=3)
    batch = {'x_t': x.to(DEV), 'cond': c.to(DEV)}
    calls = []
    monkeypatch.setattr(pn._PoseNetTrain, 'apply', lambda *a: calls.append(1) or (_ for _ in ()).throw(AssertionError))
    with torch.no_grad():
        y_train_nograd = net.train()(batch, t.to(DEV))
    y_eval_grad = net.eval()(batch, t.to(DEV))
    with torch.no_grad():
        y_eval = net.eval()(batch, t.to(DEV))
    assert not calls
    assert y_eval_grad.grad_fn is None
    assert torch.equal(y_train_nograd, y_eval) and torch.equal(y_eval_grad, y_eval)
    monkeypatch.undo()
    # the TrajNet diffusion keeps refusing
    from rohm_amd.diffusion.gaussian_diffusion_trajnet import GaussianDiffusionTrajNet
    from rohm_amd.diffusion.ddpm import LossType, ModelMeanType, ModelVarType
    td = GaussianDiffusionTrajNet(betas=np.linspace(1e-4, 0.02, 10), model_mean_type=ModelMeanType.START_X,
                                  model_var_type=ModelVarType.FIXED_SMALL, loss_type=LossType.MSE)
    with pytest.raises(NotImplementedError, match='only PoseNet training is native'):
        td.training_losses(None, {}, None)
    # shapes outside the supported set
    net.train()
    long_x = torch.randn(1, 294, 1, 150, device=DEV)
    with pytest.raises(_lib.RohmHipError, match='T=150'):
        net({'x_t': long_x, 'cond': long_x}, torch.zeros(1, dtype=torch.int64, device=DEV))
    small = PoseNet(DS(), 294, latent_dim=256, ff_size=1024, num_layers=1, num_heads=4, traj_feat_dim=22,
                    body_model_path=torch.nn.Identity(), device=DEV).to(DEV).train()
    with pytest.raises(_lib.RohmHipError, match='d_model=256'):
        small({'x_t': x[:, :, :, :8].to(DEV), 'cond': c[:, :, :, :8].to(DEV)}, t.to(DEV))
