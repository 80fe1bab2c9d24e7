"""GPU: no entry point may depend on what its workspace, scratch, saved buffer or output tensor held before the call
(include/rohm_hip.h, "Caller-owned memory").

Every wrapper of rohm_amd hands the library torch.empty memory.  In a fresh test process that memory is zero pages; in
production it is recycled activations, tags of another shape, the NaN of a diverged step.  Here torch.empty / empty_like /
Tensor.new_empty are replaced (tests/stale_memory.py) by versions that fill what they return with all-ones bytes (NaN, -1),
0x01010101 (a denormal, a small integer, a winner of atomicMin) or 0x7F7FFFFF (FLT_MAX), and every case -- one entry point
through its Python wrapper, handles built fresh inside the case because they cache workspaces -- must return, BIT FOR BIT, what
it returns from zero-filled memory, with a clean exchange status.  Outputs are compared as bytes, so NaN compares too.

Rule (b): a case whose two zero-filled runs differ from each other (free summation order: float atomicAdd) cannot be held
to bit equality; its poisoned outputs must then pass the assertion its own test makes against the oracle (ORACLE below).
Cases that use rule (b): none -- on MI355X every case of this module repeats bit for bit from zero-filled memory (the
skating counts are sums of 0 / 1, exact in any order), and the test FAILS for a case that does not repeat and has no entry
in ORACLE, so the rule cannot be used silently.

Further down: the same workspace ADDRESS used by a sequence of shapes without clearing (a caching allocator's behaviour made
deterministic: `_Recycler`), and f(x1) then f(x2) on one handle against f(x2) on a fresh one (state carried between calls).

Decisions about regions a call leaves unwritten (all documented in include/rohm_hip.h):
  * `ops.output_process` writes channels ch_off .. ch_off + C_out of `out` only (the trajectory channels are another
    kernel's): the wrapper allocates `out` with torch.zeros, and the case compares the whole tensor.
  * SMPLXLayer.forward returns joints [N, 127, 3] whose rows 22.. (55.. with vertices) are zeros from torch.zeros.
  * nothing else: every other output tensor is written in full, pad rows and unwanted optional outputs (NULL) included.

Shapes: the smallest that take every path of the big ones -- PoseNet with L <= 2 layers (d_model 512: the exchanging
launches need its 4 / 8 column tiles), TrajNet with mid_dim = 256, the smallest the library takes; at that width the
level-0 blocks AND dec[0] have 32 channels, less than the 64-wide K chunk (at the released mid_dim = 512 only dec[0] has),
which is where the clip-resident step used to read 32 floats past every row of its block-0 activation.
Found with this module (pattern all-ones; the other two patterns pass, 0 x finite being 0): every trajnet_forward / trajnet_loop
case at mid_dim 256, both loop forms, first element of every output NaN.  Two causes, both row loads of a whole 64-float K chunk
from rows that hold 32 channels: the block-0 activation of 32-channel residual blocks (level 0 and dec[1] at mid_dim 256, dec[0]
at every width), whose last row load ran past the buffer, and the input of cond_downsample1, a 32-column slice of a 64-wide row
whose neighbour columns are written later.  Fixed in csrc/trajnet*.hip by 64-wide rows with pad columns cleared once per call
(Scratch::hp).  At the released mid_dim 512 only dec[0] over-read, into memory the cond encoder of the same call has written:
finite whatever the workspace held, so the `mid 512` cases pass before and after (they pin the released width).
Reference work: model/posenet.py, model/trajnet.py, model/heads.py (what the entry points compute is pinned by their own tests)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import header_cases as HC
import stale_memory as SM
from helpers import PoseDataset, seeded
from rohm_amd.utils import synth

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TRAJ_MID = 256          # smallest mid_dim of rohm_trajnet_create; dec[0] (and level 0) has 32 channels here

CASES = {}              # name ('family[variant]') -> callable returning [(label, tensor), ...]
HANDLES = {}            # name -> (make() -> handle, call(handle, k) -> [(label, tensor), ...]) for cases whose handle caches buffers
ORACLE = {}             # name -> check(outputs): rule (b), only for cases whose zero-filled runs differ from each other


def family(name):
    return name.split('[')[0]


def case(name):
    def deco(fn):
        assert name not in CASES
        CASES[name] = fn
        return fn
    return deco


def handle_case(name, make, call):
    """A case whose handle caches a buffer: the case itself is call(make(), 0); the carried-state test runs call(h, 0), call(h, 1)."""
    assert name not in CASES
    HANDLES[name] = (make, call)
    CASES[name] = lambda: call(make(), 0)


def _d(t):
    return t.to(DEV)


# ================================================================================================ building blocks (ops)
def _ln_args(M, N, K):
    a, w = seeded(M + N, M, K), seeded(K + 7, N, K) / math.sqrt(K)
    bias, res = seeded(3, N), seeded(4, M, N) * 2 + 0.3
    g, b = seeded(5, N) * 0.5 + 1.0, seeded(6, N)
    return [_d(t) for t in (a, w, bias, res, g, b)]


def _ln_call(args, scratch, nbytes, out):
    from rohm_amd._lib import check, lib, ptr, stream_ptr
    a, w, bias, res, g, b = args
    M, K = a.shape
    N = w.shape[0]
    check(lib().rohm_gemm_res_layernorm_f32(ptr(a), K, ptr(w), K, ptr(out), N, M, N, K, ptr(bias), ptr(res), N, ptr(g), ptr(b), 1e-5,
                                            ptr(scratch), nbytes, stream_ptr(a.device)), 'rohm_gemm_res_layernorm_f32')


def _gemm_res_layernorm(M, N, K):
    """Through the wrapper, then twice more on ONE scratch (the second call meets the first one's armed header and tags)."""
    from rohm_amd import ops
    from rohm_amd._lib import lib
    args = _ln_args(M, N, K)
    out, scratch = ops.gemm_res_layernorm(*args, return_scratch=True)
    nbytes = lib().rohm_gemm_res_layernorm_scratch_bytes(M, N)
    o2, o3 = torch.empty_like(out), torch.empty_like(out)
    _ln_call(args, scratch, nbytes, o2)
    _ln_call(args, scratch, nbytes, o3)
    torch.cuda.synchronize()
    assert int(scratch[0]) == 0, 'exchange error word'
    return [('out', out), ('second call', o2), ('third call', o3)]


for _M, _N, _K in ((288, 512, 64), (144, 1024, 32)):      # 8 column tiles of 64 / of 128: the tiles really exchange
    case(f'gemm_res_layernorm[{_M}x{_N}x{_K}]')(lambda M=_M, N=_N, K=_K: _gemm_res_layernorm(M, N, K))


def _output_process(B):
    from rohm_amd import ops
    T, D, Cc = 143, 512, 272
    h, w, b = seeded(B, B * (T + 1), D) * 2 + 0.1, seeded(B + 1, Cc, D) / math.sqrt(D), seeded(B + 2, Cc)
    out, scratch = ops.output_process(_d(h), _d(w), _d(b), B, T, ch_off=22, c_total=294, return_scratch=True)
    torch.cuda.synchronize()
    assert int(scratch[0]) == 0, 'stream-K exchange error word'
    plain = ops.output_process(_d(h), _d(w), _d(b), B, T, ch_off=22, c_total=294, stream_k=False)
    return [('out', out), ('plain tiles', plain)]


for _B in (32, 3):                                          # 32: the smallest stream-K plan (tests/test_gpu_kernels.py); 3: plain tiles
    case(f'output_process[B{_B}]')(lambda B=_B: _output_process(B))


@case('attention[144x4x128]')
def _attention():
    from rohm_amd import ops
    qkv = _d(seeded(7, 144, 3 * 4 * 128))
    return [('ctx', ops.attention(qkv, 1, 4))]


@case('attention[general 2x50x64]')
def _attention_general():
    from rohm_amd import ops
    qkv = _d(seeded(8, 2 * 50, 3 * 2 * 64))
    return [('ctx', ops.attention(qkv, 2, 2, n_tok=50, head_dim=64))]


@case('layernorm[144x512]')
def _layernorm():
    from rohm_amd import ops
    x = torch.empty(144, 512, device=DEV)
    x.copy_(seeded(9, 144, 512) * 3 + 0.5)
    return [('x', ops.layernorm_(x, _d(seeded(1, 512)), _d(seeded(2, 512))))]


def _planes(mode):
    """split, GEMM on planes (fp32 + plane output), the LayerNorm-folding GEMM as producer and as consumer, LayerNorm and
    attention with plane outputs: one whole-clip shape, M = 144."""
    from rohm_amd import ops
    M, N, K = 144, 512, 512
    ws = 256.0 if mode == 16 else 1.0
    a, w, bias, res = seeded(M + N, M, K), seeded(K + 7, N, K) / math.sqrt(K), seeded(3, N), seeded(4, M, N)
    ap, wp = ops.planes_split(_d(a), mode), ops.planes_split(_d(w), mode, scale=ws)
    out = [('a planes', ap), ('w planes', wp)]
    c, cp = ops.gemm_planes(ap, wp, M, N, K, mode, _d(bias), None, 1, out_planes=True, acc_scale=1.0 / ws)
    out += [('gelu gemm', c), ('gelu gemm planes', cp)]
    if mode != 3:
        c2, cp2, st = ops.gemm_planes_ln(ap, wp, M, N, K, mode, _d(bias), _d(res), 2, acc_scale=1.0 / ws, want_stats=True, ln_dim=N,
                                         out_planes=True)
        out += [('ln producer', c2), ('ln producer planes', cp2), ('ln producer stats', st)]
        g = a.double().reshape(M // 16, 16, K // 16, 16)
        stats = torch.stack([g.sum(-1), (g * g).sum(-1)], -1).permute(0, 2, 1, 3).contiguous().float()
        c3, _, _ = ops.gemm_planes_ln(ap, wp, M, N, K, mode, _d(bias), None, 1, acc_scale=1.0 / ws, ln_stats=_d(stats),
                                      ln_c=_d(w.sum(1)), ln_dim=K)
        out += [('ln consumer', c3)]
    x = _d(seeded(5, M, 512) * 3 + 0.5)
    out += [('layernorm planes', ops.layernorm_planes_(x, _d(seeded(1, 512)), _d(seeded(2, 512)), mode)), ('layernorm', x)]
    out += [('attention planes', ops.attention_planes(_d(seeded(7, 144, 3 * 4 * 128)), 1, 4, mode))]
    return out


for _mode in (3, 16):
    case(f'planes[mode {_mode}]')(lambda mode=_mode: _planes(mode))


@case('ddpm[step, table, dropout mask]')
def _ddpm():
    from rohm_amd import ops
    from rohm_amd.model.posenet import dropout_mask
    B, n = 3, 294 * 143
    x, x0, nz, ga = (_d(seeded(s, B, 294, 1, 143)) for s in (1, 2, 3, 4))
    out = [('ddpm_step', ops.ddpm_step(x, x0, nz, 0.3, 0.7, 0.1, grad=ga, grad_scale=2.0))]
    tables = _d(seeded(5, 10, 4))
    t = torch.tensor([0, 9, 4], device=DEV)
    out += [('ddpm_step_table', ops.ddpm_step_table(x, x0, nz, tables, t, grad_a=ga, w_a=3.0))]
    out += [('dropout mask', dropout_mask(1234, 0, 2, (2, 64, 512), 0.1, DEV).to(torch.uint8)),
            ('dropout mask odd', dropout_mask(99, 1, 1, (1, 4, 13, 13), 0.5, DEV).to(torch.uint8))]
    return out


# ================================================================================================ PoseNet
_POSE_ENV = {'0': dict(ROHM_POSENET_CHAIN='0', ROHM_POSENET_CHAIN_ANY=None),
             'layer': dict(ROHM_POSENET_CHAIN='layer', ROHM_POSENET_CHAIN_ANY='1'),
             'stack': dict(ROHM_POSENET_CHAIN='stack', ROHM_POSENET_CHAIN_ANY='1')}


def _body(num_verts=433):
    from rohm_amd.body_model import SMPLXLayer
    return SMPLXLayer.from_tensors(synth.synthetic_smplx_tensors(0, num_verts=num_verts))


def _make_posenet(chain, L=2, body=None, stats=None, dropout=0.1):
    """PoseNet with L layers whose native handle was created under the chain form `chain` (the handle reads the environment at
    create; tests/test_gpu_chain.py::_pair)."""
    from rohm_amd.model.posenet import PoseNet
    ds = PoseDataset(*(stats or (None, None)))
    ds.cam_R, ds.cam_t = torch.tensor(synth.SYNTH_CAM_R), torch.tensor(synth.SYNTH_CAM_T)
    net = PoseNet(ds, 294, latent_dim=512, ff_size=1024, num_layers=L, num_heads=4, traj_feat_dim=22, dropout=dropout,
                  body_model_path=body if body is not None else torch.nn.Identity(), device=DEV)
    net.load_state_dict(synth.posenet_state_dict(5, num_layers=L), strict=False)
    net = net.to(DEV).eval()
    if chain is not None:
        with SM.env(**_POSE_ENV[chain]):
            net.native(torch.device(DEV))
    return net


def _pose_inputs(B, T, k=0):
    x, c = _d(seeded(1 + 10 * k, B, 294, 1, T)), _d(seeded(2 + 10 * k, B, 294, 1, T))
    t = torch.tensor([(37 * i + 1 + 100 * k) % 1000 for i in range(B)], device=DEV)
    return x, c, t


def _pose_forward(net, B, T, k=0):
    x, c, t = _pose_inputs(B, T, k)
    y = net({'x_t': x, 'cond': c}, t)
    net.check_exchange()
    return [('out', y)]


def _pose_loop(net, B, T, k=0, n=8):
    x, c, _ = _pose_inputs(B, T, k)
    noise = _d(seeded(3 + 10 * k, n, B, 294, 1, T))
    coef = np.asarray([[0.05 + 0.01 * i, 0.95 - 0.01 * i, 0.1] for i in range(n)], np.float32)
    ts = [400 - 3 * i for i in range(n)]
    x_in = torch.empty_like(x)
    x0 = net.sample_loop_native(x, c, ts, coef, noise, want_x0_last=True, x_in_last=x_in)
    net.check_exchange()
    return [('x', x), ('x0 of the last step', x0), ('input of the last step', x_in)]


for _chain in ('0', 'layer', 'stack'):
    for _B, _T in ((1, 143), (3, 143), (3, 63)):            # T = 63: the path for clips that are not 144 tokens
        handle_case(f'posenet_forward[chain {_chain}, B{_B}, T{_T}]', lambda ch=_chain: _make_posenet(ch),
                    lambda net, k, B=_B, T=_T: _pose_forward(net, B, T, k))
    handle_case(f'posenet_loop[chain {_chain}, B3, T143, 8 steps]', lambda ch=_chain: _make_posenet(ch),
                lambda net, k: _pose_loop(net, 3, 143, k))


def _make_guided():
    stats = synth.synthetic_stats(0)
    return _make_posenet('0', body=_body(), stats=stats), stats


def _pose_guided(h, k=0):
    """One guided ancestral step (t = 10 <= 50: skating guidance with the reference's weight) through the diffusion engine."""
    from test_gpu_posenet import make_diffusion
    net, (mean, std) = h
    B, T = 2, 143
    cond = _d(synth.plausible_motion(30 + k, B, T, mean, std))
    x = _d(synth.plausible_motion(31 + k, B, T, mean, std) + 0.05 * seeded(3 + k, B, 294, 1, T))
    nz = _d(seeded(4 + k, B, 294, 1, T))
    diff = make_diffusion(1000)
    diff.noise_source = lambda step, like: nz
    out = diff.p_sample_with_grad(net, {'cond': cond}, x, torch.full((B,), 10, device=DEV, dtype=torch.int64), grad_type='amass')
    net.check_exchange()
    return [('sample', out['sample']), ('pred_xstart', out['pred_xstart'])]


handle_case('posenet_guided[amass, t 10]', _make_guided, _pose_guided)


def _posenet_train(T, p):
    """rohm_posenet_train_forward / _backward through autograd: the output, the input gradients and EVERY parameter gradient (the
    slices of the flat gradient buffer)."""
    from rohm_amd.model.posenet import train_param_names
    net = _make_posenet(None, L=1, dropout=p).train()
    B = 2
    x, c, t = _pose_inputs(B, T)
    x.requires_grad_()
    c.requires_grad_()
    torch.manual_seed(3)
    y = net({'x_t': x, 'cond': c}, t)
    y.backward(_d(seeded(4, B, 294, 1, T)))
    out = [('out', y), ('d_x_t', x.grad), ('d_cond', c.grad)]
    for name, q in zip(train_param_names(1), net.train_parameters()):
        assert q.grad is not None, name
        out.append(('d ' + name, q.grad))
    return out


for _T in (63, 143):
    for _p in (0.0, 0.1):
        case(f'posenet_train[L1, B2, T{_T}, dropout {_p}]')(lambda T=_T, p=_p: _posenet_train(T, p))


# ================================================================================================ TrajNet
def _make_trajnet(ctrl, mid=TRAJ_MID, train=False):
    from rohm_amd.model.trajnet import TrajNet
    net = TrajNet(time_dim=32, mid_dim=mid, cond_dim=13, traj_feat_dim=13, trajcontrol=ctrl, device=DEV)
    net.load_state_dict(synth.trajnet_state_dict(11, mid_dim=mid, trajcontrol=ctrl), strict=True)
    net = net.to(DEV)
    return net.train() if train else net.eval()


def _traj_batch(B, T, k=0):
    return {'x_t': _d(seeded(1 + 10 * k, B, T, 13)), 'cond': _d(seeded(2 + 10 * k, B, T, 13)),
            'control_cond': _d(seeded(3 + 10 * k, B, T, 272))}


def _traj_forward(net, B, T, k=0):
    t = torch.tensor([(37 * i + 3 + 7 * k) % 100 for i in range(B)], device=DEV)
    return [('out', net(_traj_batch(B, T, k), t))]


def _traj_loop(net, resident, B, T, k=0, n=4):
    from rohm_amd._lib import lib
    batch = _traj_batch(B, T, k)
    x = batch['x_t']
    noise = _d(seeded(4 + 10 * k, n, B, T, 13))
    coef = np.asarray([[0.05 + 0.01 * i, 0.95 - 0.01 * i, 0.1] for i in range(n)], np.float32)
    x_in = torch.empty_like(x)
    with SM.env(ROHM_TRAJ_RESIDENT=resident):
        x0 = net.sample_loop_native(x, batch['cond'], [60 - 2 * i for i in range(n)], coef, noise, want_x0_last=True, batch=batch,
                                    x_in_last=x_in)
    torch.cuda.synchronize()
    msg = lib().rohm_last_error()
    assert not (msg and b'clip-resident step did not complete' in msg), msg      # a fallback is a finding, not a pass
    # the form the case is named after really ran (the resident builder refuses a layer it cannot run and the call then falls through,
    # silently, to one launch per layer)
    assert lib().rohm_trajnet_loop_mode() == int(resident), (resident, B, T)
    return [('x', x), ('x0 of the last step', x0), ('input of the last step', x_in)]


for _ctrl in (False, True):
    _tag = 'TrajControl' if _ctrl else 'TrajNet'
    for _B, _T in ((1, 16), (9, 48), (9, 144)):             # B = 9: two clips on one XCD in the resident form
        handle_case(f'trajnet_forward[{_tag}, B{_B}, T{_T}]', lambda c=_ctrl: _make_trajnet(c),
                    lambda net, k, B=_B, T=_T: _traj_forward(net, B, T, k))
        for _res in ('1', '0'):                               # clip-resident step / one launch per layer
            handle_case(f'trajnet_loop[{_tag}, resident {_res}, B{_B}, T{_T}, 4 steps]', lambda c=_ctrl: _make_trajnet(c),
                        lambda net, k, r=_res, B=_B, T=_T: _traj_loop(net, r, B, T, k))


# the released width: only dec[0] (32 channels) is narrower than the K chunk there
handle_case('trajnet_forward[TrajNet, mid 512, B9, T48]', lambda: _make_trajnet(False, mid=512), lambda net, k: _traj_forward(net, 9, 48, k))
for _res in ('1', '0'):
    handle_case(f'trajnet_loop[TrajNet, mid 512, resident {_res}, B9, T48, 4 steps]', lambda: _make_trajnet(False, mid=512),
                lambda net, k, r=_res: _traj_loop(net, r, 9, 48, k))


def _trajnet_train(ctrl, frozen):
    """rohm_trajnet_train_forward / _backward (mid_dim 512: the training path's one width).  `frozen`: only the ControlNet branch
    trains, the backbone's gradient pointers are NULL."""
    net = _make_trajnet(ctrl, mid=512, train=True)
    if frozen:
        for name, q in net.named_parameters():
            q.requires_grad_(name.startswith('controlnet.'))
    B, T = 2, 16
    y = net(_traj_batch(B, T), torch.tensor([3, 77], device=DEV))
    y.backward(_d(seeded(9, B, T, 13)))
    out = [('out', y)]
    for name, q in net.named_parameters():
        if frozen and not name.startswith('controlnet.'):
            assert q.grad is None, name
        elif q.grad is not None:
            out.append(('d ' + name, q.grad))
    assert len(out) > 50
    return out


case('trajnet_train[TrajNet, B2, T16]')(lambda: _trajnet_train(False, False))
case('trajnet_train[TrajControl, B2, T16]')(lambda: _trajnet_train(True, False))
case('trajnet_train[TrajControl, frozen backbone, B2, T16]')(lambda: _trajnet_train(True, True))


# ================================================================================================ body model and guidance
class _GuidanceModel:
    """What rohm_amd.guidance reads of a PoseNet: the body model and the dataset statistics."""

    def __init__(self):
        mean, std = synth.synthetic_stats(2)
        self.dataset = PoseDataset(mean, std)
        self.dataset.cam_R, self.dataset.cam_t = torch.tensor(synth.SYNTH_CAM_R), torch.tensor(synth.SYNTH_CAM_T)
        self.smplx_model = _body().to(DEV)
        self.stats = (mean, std)


def _motion(m, B, T, k):
    return _d(synth.plausible_motion(22 + 5 * k, B, T, *m.stats, angle_scale=2.5 if k == 0 else 0.4))


def _guide_skating(m, k=0, split=False):
    from rohm_amd.guidance import guide_skating
    B, T = 2, 50                                               # the smallest (B, T) of tests/test_gpu_guidance.py
    if split:
        m.guidance_group = lambda t: t                         # prepare + all-reduce (identity) + apply
    grad, counts = guide_skating(m, {}, {'pred_xstart': _motion(m, B, T, k)}, None, 'x_0', return_counts=True)
    return [('grad', grad), ('counts2', counts)]


def _guide_proj2d(m, k=0):
    from rohm_amd.guidance import guide_2d_projection
    B, T = 2, 50
    cam = {n: _d(v) for n, v in synth.synthetic_camera_batch(k, B).items()}
    return [('grad', guide_2d_projection(m, cam, {'pred_xstart': _motion(m, B, T, k)}, None, 'x_0'))]


handle_case('guidance_skating[B2, T50]', _GuidanceModel, lambda m, k: _guide_skating(m, k))
handle_case('guidance_skating_split[B2, T50]', _GuidanceModel, lambda m, k: _guide_skating(m, k, split=True))
handle_case('guidance_proj2d[B2, T50]', _GuidanceModel, _guide_proj2d)


def _make_lbs(skin):
    from rohm_amd.body_model import native_for
    body = _body().to(DEV)
    with SM.env(ROHM_LBS_SKIN=skin):
        nat = native_for(body, DEV)
    assert nat.has_lbs and int(_lib().rohm_smplx_skinning_mode(nat.handle)) == {'mfma': 0, 'sparse': 1}[skin]
    return body, nat


def _lib():
    from rohm_amd._lib import lib
    return lib()


def _lbs(h, N, verts, k=0):
    from rohm_amd.body_model import lbs_forward
    _, nat = h
    pose, betas, transl = _d(seeded(1 + k, N, 22, 3) * 0.4), _d(seeded(2 + k, N, 10)), _d(seeded(3 + k, N, 3))
    joints, v = lbs_forward(nat, pose, 0, betas, transl, want_verts=verts)
    return [('joints', joints)] + ([('verts', v)] if verts else [])


for _skin in ('mfma', 'sparse'):                               # mfma: the dense mode, whose transform rows are cleared by a memset
    for _N in (1, 17):                                         # 17: a part-filled second group of 16 and a part-filled tile of 144
        for _verts in (True, False):
            handle_case(f'smplx_forward[{_skin}, N{_N}, {"verts" if _verts else "joints only"}]', lambda s=_skin: _make_lbs(s),
                        lambda h, k, N=_N, v=_verts: _lbs(h, 17 if (k and N == 1) else (1 if k else N), v, k))


@case('smplx_joints[N17]')
def _smplx_joints():
    body = _body().to(DEV)
    N = 17
    out = body(betas=_d(seeded(1, N, 10)), global_orient=_d(seeded(2, N, 3) * 0.8), body_pose=_d(seeded(3, N, 63) * 0.5),
               transl=_d(seeded(4, N, 3)))
    return [('joints', out.joints)]


# ================================================================================================ clips and data entry points
def _recording(N=40):
    jw, world = synth.synthetic_recording(3, N, 'z')
    return _d(torch.from_numpy(jw)), _d(torch.from_numpy(world))


def _clips(f64, stats):
    from rohm_amd.data_loaders.clips import build_clips
    jw, world = _recording()
    out = build_clips(jw, world, 16, 2, 'z', None, stats=synth.synthetic_stats(0) if stats else None, params_f64=f64)
    return sorted(out.items())


case('clips_build[N40, L16]')(lambda: _clips(False, False))
case('clips_build[N40, L16, normalised]')(lambda: _clips(False, True))
case('clips_build_f64[N40, L16]')(lambda: _clips(True, False))


@case('clips_repr[C2, L16, joint noise]')
def _clips_repr():
    from rohm_amd.data_loaders.clips import build_clips, clips_repr
    jw, world = _recording()
    with SM.poison(SM.ZEROS):                                  # (the inputs of the call under test come from clean memory)
        b = build_clips(jw, world, 16, 2, 'z', None, params_f64=True)
    n, L = b['cano_joints'].shape[:2]
    idx = (b['starts'].long()[:, None] + torch.arange(L, device=DEV)[None]).reshape(-1)
    params = world[idx].reshape(n, L, 79).clone()
    params[:, :, :6] = b['orient_transl64']
    noise = _d(seeded(5, n, L, 22, 3).double() * 0.01)
    rep, joints = clips_repr(b['cano_joints'].double(), params, stats=synth.synthetic_stats(0), joint_noise=noise, return_joints=True)
    plain = clips_repr(b['cano_joints'], params)
    return [('repr', rep), ('joints', joints), ('repr of float32 joints', plain)]


@case('repr_stats[rows 2 x 15 and 7000]')
def _repr_stats():
    from rohm_amd.data_loaders.dataloader_amass import repr_stats
    out = []
    for tag, x in (('small', seeded(1, 2, 15, 294)), ('large', seeded(2, 7000, 294) * 2 + 0.5)):
        mean, std = repr_stats(_d(x))
        out += [(tag + ' mean', mean), (tag + ' std', std)]
    return out


@case('keypoints[undistort, visibility masks]')
def _keypoints():
    from rohm_amd.data_loaders.clips import undistort_keypoints, visibility_masks
    N = 40
    kp = seeded(1, N, 22, 3).abs() * torch.tensor([900.0, 500.0, 0.4])
    und = undistort_keypoints(_d(kp), [[1060.53, 0.0, 951.30], [0.0, 1060.38, 536.77], [0.0, 0.0, 1.0]],
                              [0.052, -0.044, 0.0009, 0.0016, 0.003])
    mask = (seeded(2, N, 25) > 0).float()
    jv, vv = visibility_masks(_d(kp), _d(mask), 16, 2)
    return [('undistorted', und), ('mask_joint_vis', jv), ('mask_vec_vis', vv)]


# ================================================================================================ rendering
def _scene():
    """tests/raster_scenes.py's scene (a wall, a table; nothing on the far left: pixels no triangle covers) and a second copy of it
    moved back, seen through PROX's camera at 1 / 20 of its resolution."""
    import raster_ref as rr
    from raster_scenes import scene_mesh
    v, f = scene_mesh()
    verts = np.stack([v, v + np.array([0.25, 0.0, 0.5], np.float32)])
    cam = tuple(x / 20.0 for x in rr.PROX_CAM)
    return _d(torch.from_numpy(verts)), f, cam, (96, 54)


@case('depth[render, probe, project, occlusion mask]')
def _depth():
    from rohm_amd import occlusion
    verts, faces, cam, size = _scene()
    depth = occlusion.depth_render(verts, faces, cam, size)
    assert bool((depth == 0).any()) and bool((depth > 0).any()), 'the scene must leave pixels uncovered'
    culled = occlusion.depth_render(verts[0], faces, cam, size, cull_backfaces=True)
    joints = _d(seeded(1, 2, 25, 3) * torch.tensor([1.5, 0.8, 0.5]) + torch.tensor([0.0, 0.0, 2.5]))
    pix = occlusion.project_pixels(joints, occlusion.camera_matrix(cam), [0.052, -0.044, 0.0009, 0.0016, 0.003])
    probe = occlusion.depth_probe(verts, faces, pix, cam, size)
    mask = occlusion.mask_from_depths(joints, depth[0], probe, occlusion.camera_matrix(cam))
    return [('depth', depth), ('depth, culled', culled), ('pixels', pix), ('probe', probe), ('mask', mask)]


@case('color[render with depth and face id, normals, skeleton mesh]')
def _color():
    from rohm_amd import render
    verts, faces, cam, size = _scene()
    V = verts.shape[1]
    colors = _d((seeded(1, V, 4).abs() * 100).clamp(0, 255).to(torch.uint8))
    normals = render.vertex_normals(verts, faces)
    rgba, depth, fid = render.color_render(verts, faces, colors, cam, size, normals=normals, with_depth=True, with_face_id=True)
    assert bool((fid == -1).any()) and bool((fid >= 0).any()), 'the scene must leave pixels uncovered'
    flat = render.color_render(verts, faces, colors, cam, size)
    sphere, _ = render.icosphere(1)
    cyl, _ = render.cylinder(8)
    joints = _d(seeded(2, 3, 22, 3))
    hide = (seeded(3, 3, 22 + 21) > 1.0).to(torch.uint8)
    skel = render.skeleton_mesh(joints, sphere, cyl, hide=_d(hide))
    return [('normals', normals), ('rgba', rgba), ('depth', depth), ('face id', fid), ('rgba, flat', flat), ('skeleton', skel)]


# ================================================================================================ representation, export, data, metrics
def _repr_batch(B=2, T=20, seed=7):
    mean, std = synth.synthetic_stats(0)
    x = synth.plausible_motion(seed, B, T, mean, std)                      # [B, 294, 1, T], normalised
    return _d(x), (mean, std)


@case('repr[frames_to_world, joints, joints vjp, rederive]')
def _repr():
    from rohm_amd.data_loaders import motion_representation as mr
    from rohm_amd.data_loaders.frames import frames_to_world, noisy_clip_joints
    body = _body().to(DEV)
    N = 17
    params = {'global_orient': seeded(1, N, 3) * 0.8, 'body_pose': seeded(2, N, 63) * 0.3, 'betas': seeded(3, N, 10), 'transl': seeded(4, N, 3)}
    cam2world = np.eye(4, dtype=np.float32)
    cam2world[:3, :3] = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    cam2world[:3, 3] = (0.5, -0.25, 1.0)
    jw, world = frames_to_world(body, params, cam2world, device=DEV)
    out = [('joints_world', jw), ('smplx_world', world), ('noisy clip joints', noisy_clip_joints(body, params, device=DEV))]
    x, stats = _repr_batch()
    for mode in ('smplx_params', 'joint_abs_traj', 'joint_rel_traj'):
        j = mr.joints_from_repr(x, mode, smplx_model=body, stats=stats, layout='bc1t')
        dx = mr.joints_vjp(x, _d(seeded(9, *j.shape)), mode, smplx_model=body, stats=stats, layout='bc1t')
        out += [('joints ' + mode, j), ('vjp ' + mode, dx)]
    xb = x[:, :, 0].permute(0, 2, 1).contiguous()                           # [B, T, 294]
    out.append(('rederived trajectory', mr.rederive_traj(xb, stats, stats, body)))
    cond = torch.empty(2, 294, 1, 19, device=DEV)                           # channels 0..21 are written in place, the rest is the caller's
    cond.copy_(_d(seeded(5, 2, 294, 1, 19)))
    out.append(('rederived into cond', mr.rederive_traj(xb, stats, stats, body, out=cond, out_layout='bc1t')))
    return out


@case('export_smplx[with and without contact, out-of-range frame]')
def _export():
    from rohm_amd import ops
    from rohm_amd.body_model import native_for
    body = _body().to(DEV)
    x, (mean, std) = _repr_batch()
    clip = torch.tensor([0, 1, 1, 0, 5], dtype=torch.int32, device=DEV)    # clip 5 does not exist: a NaN row
    row = torch.tensor([0, 3, 19, 7, 0], dtype=torch.int32, device=DEV)
    transf = torch.eye(4, device=DEV).repeat(2, 1, 1).contiguous()
    transf[:, :3, 3] = torch.tensor([0.5, -1.0, 0.25], device=DEV)
    h = native_for(body, DEV).handle
    params, contact = ops.export_smplx(h, x, 'bc1t', clip, row, transf=transf, rigid=torch.eye(4, dtype=torch.float64, device=DEV),
                                       mean=_d(torch.from_numpy(mean)), std=_d(torch.from_numpy(std)))
    plain, none = ops.export_smplx(h, x, 'bc1t', clip, row, want_contact=False)
    assert none is None
    return [('params', params), ('contact', contact), ('params, no transforms', plain)]


@case('amass[batch assembly, parameter noise, preprocessing]')
def _amass():
    from rohm_amd import preprocessing_amass as pa
    from rohm_amd.data_loaders.dataloader_amass import assemble, param_noise
    mean, std = (_d(torch.from_numpy(a)) for a in synth.synthetic_stats(0))
    clean, noisy = _d(seeded(1, 6, 15, 294)), _d(seeded(2, 6, 15, 294))
    idx = torch.tensor([4, 0, 5], device=DEV)
    out = []
    for tag, kw in (('pose', dict(overwrite_channels=22, cond='traj', control=True)), ('traj', dict(cond='abs')), ('plain', {})):
        out += [(f'{tag} {k}', v) for k, v in sorted(assemble(clean, noisy, idx, mean, std, **kw).items())]
    out += [(f'per batch {k}', v) for k, v in sorted(assemble(clean, noisy[:3].contiguous(), idx, mean, std, noisy_per_batch=True).items())]
    p = _d(seeded(3, 2, 5, 79).double() * 0.3)
    nz = {'global_orient': _d(seeded(4, 2, 5, 3).double()), 'transl': _d(seeded(5, 2, 5, 3).double() * 0.01),
          'betas': _d(seeded(6, 2, 5, 10).double() * 0.1), 'body_pose': _d(seeded(7, 2, 5, 63).double())}
    out += [('param noise', param_noise(p, nz)), ('param noise, additive', param_noise(p, nz, additive=True))]
    N = 17
    arrays = {k: _d(seeded(10 + i, N, d).double() * 0.3) for i, (k, d) in enumerate(pa.FRAME_KEYS)}
    joints, params = pa.preprocess_frames(_body().to(DEV), arrays, _d(seeded(20, 2, 10).double()), np.arange(N) % 2)
    return out + [('preprocessed joints', joints), ('preprocessed params', params)]


@case('track_resample[gaps, keypoints, masks]')
def _track():
    from rohm_amd.data_loaders.track import resample_track
    N = 40
    g = np.random.Generator(np.random.PCG64(5))
    times = np.cumsum(g.uniform(0.02, 0.06, size=N))
    valid = g.uniform(size=N) > 0.25
    valid[[0, N - 1]] = True
    valid[10:17] = False                                                      # a gap longer than max_gap
    out = resample_track(times, valid, seeded(1, N, 79).double().numpy() * 0.3, keypoints=seeded(2, N, 22, 3).numpy(),
                         mask_joint=(seeded(3, N, 25) > 0).float().numpy(), device=DEV)
    bare = resample_track(times, valid, seeded(1, N, 79).double().numpy() * 0.3, device=DEV)
    return [(k, v) for k, v in sorted(out.items())] + [('bare ' + k, v) for k, v in sorted(bare.items()) if v is not None]


@case('metrics[amass, scene, result rows, traj report]')
def _metrics():
    from rohm_amd import evaluation as ev
    from rohm_amd.drivers import results as rs
    n, T = 3, 20
    jc = _d(seeded(1, n, T, 22, 3))
    jr = jc + 0.05 * _d(seeded(2, n, T, 22, 3))
    rc, rr = _d(seeded(3, n, T, 294)), _d(seeded(4, n, T, 294))
    out = []
    for scheme, ratio in (('lower', 0.0), ('full', 0.3)):
        m = ev.amass_metrics(jc, jr, rc, rr, scheme, ratio)
        out.append((f'amass metrics {scheme}', torch.tensor([m[k] for k in sorted(m)], dtype=torch.float64)))
    tm = torch.eye(4, device=DEV).repeat(n, 1, 1).contiguous()
    sm, js = ev.scene_metrics(jr, tm, 0.1, 'prox', return_joints_scene=True)
    se = ev.scene_metrics(jr, tm, [0.1, 0.0, -0.1], 'egobody', joints_gt=_d(seeded(5, n, T + 3, 22, 3)),
                          mask_joint_vis=(_d(seeded(6, n, T, 22)) > 0).float())
    out += [('scene metrics prox', torch.from_numpy(sm.sums)), ('joints in the scene', js), ('scene metrics egobody', torch.from_numpy(se.sums))]
    stats = synth.synthetic_stats(0)
    rows = rs.result_rows([(_d(seeded(7, n, 294, 1, T)), 'bc1t'), (rc, 'btc', _d(seeded(8, n, T + 1, 22))), (rr, 'btc'), (rc, 'btc')], stats, T=T - 1)
    out += [(f'result rows {i}', r) for i, r in enumerate(rows)]
    rep, elems = rs.traj_report([jc, jr, jr * 1.01, jr * 0.99, jc + 0.01], rc, rr, return_elems=True)
    return out + [('traj report', torch.from_numpy(rep.sums)), ('traj report terms', elems)]


@case('train_helpers[cond, trajectory window, q_sample, image operators]')
def _train_helpers():
    from rohm_amd import render
    from rohm_amd.train import masks
    from test_gpu_posenet import make_diffusion
    B, T = 3, 20
    src, clean = _d(seeded(1, B, T, 294)), _d(seeded(2, B, T, 294))
    vis = np.random.Generator(np.random.PCG64(3)).integers(0, 2 ** 22, size=(4, T)).astype(np.uint32)
    cond, clean_t = masks.train_cond(src, clean, joint_bits=np.array([masks.joint_bits([1, 4, 7]), 0, masks.joint_bits(range(22))], np.uint32),
                                     window=np.array([[2, 9], [0, 0], [5, T]], np.int32), vis_bits=vis, vis_index=np.array([3, 0, 1]),
                                     zero_contact=True)
    plain, none = masks.train_cond(src)
    assert none is None
    tw = masks.traj_window(_d(seeded(4, B, T, 13)), np.array([[0, 3], [7, 7], [10, T]], np.int32), 9)
    x0 = _d(seeded(5, B, 294, 1, T))
    q = make_diffusion(1000).q_sample(x0, torch.tensor([0, 500, 999], device=DEV), noise=_d(seeded(6, B, 294, 1, T)))
    img = _d((seeded(7, 2, 9, 11, 4).abs() * 120).clamp(0, 255).to(torch.uint8))
    rgb = _d((seeded(8, 2, 9, 11, 3).abs() * 120).clamp(0, 255).to(torch.uint8))
    return [('cond', cond), ('clean transposed', clean_t), ('cond, no masks', plain), ('trajectory window', tw), ('q_sample', q),
            ('requantize', render.requantize(img, 0.5)), ('paste', render.paste(rgb, img)), ('overlay', render.overlay(rgb, img)),
            ('flip', render.flip_lr(img))]


# ================================================================================================ optimiser
@case('optim[AdamW with clipping, two steps]')
def _optim():
    """Two consecutive steps with different gradients on ONE optimiser: `_norm_out` is zeroed once and reused, the norm scratch is
    torch.empty memory."""
    from rohm_amd import optim
    shapes = [(5,), (300, 7), (1025,), (64, 64)]
    ps = [_d(seeded(i, *s)).requires_grad_() for i, s in enumerate(shapes)]
    opt = optim.AdamW(ps, lr=1e-2, max_grad_norm=1.0)
    out = []
    for step, scale in ((0, 0.01), (1, 3.0)):                  # below and above the clipping norm
        for i, (q, s) in enumerate(zip(ps, shapes)):
            q.grad = _d(seeded(100 + 10 * step + i, *s) * scale)
        opt.step()
        out += [(f'step {step} grad norm', opt.last_grad_norm.clone())] + [(f'step {step} param {i}', q.detach().clone()) for i, q in enumerate(ps)]
    return out


# ================================================================================================ the headers next to rohm_hip.h
for _name, (_, _inputs, _call) in HC.CASES.items():         # rohm_multiview.h, rohm_fit_views.h, rohm_rig.h: every declaration of each
    case(_name)(lambda i=_inputs, c=_call: c(HC.tensors(i, 7, lambda t: _d(t))))     # (`_d` as it is at the call: other modules replace it)


# ================================================================================================ the tests
def _run(fn, word):
    with SM.poison(word):
        out = fn()
        torch.cuda.synchronize()
    return SM.snapshot(out)


@pytest.mark.parametrize('name', sorted(CASES))
def test_outputs_do_not_depend_on_what_uninitialised_memory_held(name):
    """(a) bit equality with the zero-filled baseline under every pattern, wherever two zero-filled runs agree bit for bit
    (established first); (b) otherwise the case's own oracle."""
    fn = CASES[name]
    base = _run(fn, SM.ZEROS)
    assert base and all(t.numel() > 0 for _, t in base)
    repeatable = not SM.differences(_run(fn, SM.ZEROS), base)
    assert repeatable or name in ORACLE, f'{name}: two zero-filled runs differ and the case names no oracle'
    failures = {}
    for pname, word in SM.PATTERNS.items():
        got = _run(fn, word)
        if repeatable:
            diff = SM.differences(got, base)
            if diff:
                failures[pname] = diff[:3]          # (output, (first differing element, poisoned value there, baseline value))
        else:
            ORACLE[name](got)
    assert not failures, f'{name}: outputs depend on stale memory: {failures}'


@pytest.mark.parametrize('name', sorted(HANDLES))
def test_no_state_is_carried_from_one_call_to_the_next(name):
    """f(x1) then f(x2) on one handle (its cached workspace holds f(x1)'s remains) == f(x2) on a fresh handle."""
    make, call = HANDLES[name]
    with SM.poison(SM.PATTERNS['ones']):
        want = [(l, t.clone()) for l, t in call(make(), 1)]
        h = make()
        first = [(l, t.clone()) for l, t in call(h, 0)]
        got = [(l, t.clone()) for l, t in call(h, 1)]
        again = [(l, t.clone()) for l, t in call(h, 0)]
        torch.cuda.synchronize()
    assert not SM.differences(got, want), (name, SM.differences(got, want)[:3])
    assert not SM.differences(again, first), (name, SM.differences(again, first)[:3])


# ---- one address, a sequence of shapes ------------------------------------------------------------------------------------------
class _Recycler:
    """A caching allocator's recycling made deterministic: while active, the i-th flat uint8 / int32 device allocation of a call
    (the workspaces, scratch and saved buffers of every wrapper) is the front of the i-th of a few persistent 256-byte-aligned
    arenas -- the same ADDRESS call after call, shape after shape, never cleared in between.  The arenas start as all-ones bytes.

    This stands in for driving the C ABI with one aligned buffer: same addresses, same missing clears, but through the wrappers, so the
    very allocation sites production uses are the ones recycled.  It recognises them by their call form, `torch.empty(n, dtype=torch.uint8
    | torch.int32, device=...)` with one integer size; a wrapper that allocates differently would be served ordinary memory and its test
    would prove nothing -- which is why every user asserts the exact number of allocations `served`."""

    def __init__(self, nbytes, n=3):
        self.arenas = []
        for _ in range(n):
            a = torch.full((nbytes + 256,), 0xFF, dtype=torch.uint8, device=DEV)
            self.arenas.append(a[(-a.data_ptr()) % 256:][:nbytes])
        self.i = 0
        self.served = 0

    def begin(self):
        self.i = 0

    def install(self, monkeypatch):
        real = torch.empty

        def empty(*a, **k):
            dt, dev = k.get('dtype'), k.get('device')
            if dt in (torch.uint8, torch.int32) and dev is not None and torch.device(dev).type == 'cuda' and len(a) == 1 and isinstance(a[0], int):
                nbytes = a[0] * (4 if dt == torch.int32 else 1)
                arena = self.arenas[self.i]
                assert nbytes <= arena.numel(), (nbytes, arena.numel())
                self.i += 1
                self.served += 1
                return arena[:nbytes].view(dt)
            return real(*a, **k)
        monkeypatch.setattr(torch, 'empty', empty)


def _sequence(rec, steps, refs):
    """Run `steps` = [(key, thunk)]: every output must equal the reference of its key, bit for bit."""
    for n, (key, thunk) in enumerate(steps):
        rec.begin()
        got = [(l, t.clone()) for l, t in thunk()]
        torch.cuda.synchronize()
        diff = SM.differences(got, refs[key])
        assert not diff, f'call {n} ({key}) in recycled memory differs from the call in fresh zero-filled memory: {diff[:3]}'


_ABAB = ['A'] + ['B'] * 40 + ['A', 'C', 'A', 'B']           # B runs enough passes to overtake A's pass counter


@pytest.mark.parametrize('loop', [False, True])
@pytest.mark.parametrize('chain', ['layer', 'stack'])
def test_posenet_workspace_address_reused_by_other_shapes(chain, loop, monkeypatch):
    """A = (B 3, T 143), B = (B 1, T 143), C = (B 3, T 63) in ONE workspace address on one handle and stream: the exchange header,
    statistics slots and flags sit at offsets that depend on the shape, so A meets its own surviving header with slot regions that
    B's tags and activations have written in between."""
    shapes = {'A': (3, 143), 'B': (1, 143), 'C': (3, 63)}
    run = (lambda net, B, T: _pose_loop(net, B, T)) if loop else (lambda net, B, T: _pose_forward(net, B, T))
    refs = {}
    for key, (B, T) in shapes.items():
        refs[key] = _run(lambda: run(_make_posenet(chain), B, T), SM.ZEROS)
    net = _make_posenet(chain)
    nbytes = max(_lib().rohm_posenet_workspace_bytes(net.native(torch.device(DEV)).handle, B, T) for B, T in shapes.values())
    rec = _Recycler(nbytes, n=1)
    rec.install(monkeypatch)
    _sequence(rec, [(k, lambda k=k: run(net, *shapes[k])) for k in _ABAB], refs)
    assert rec.served == 6                                     # every change of shape drew the workspace again, from the arena


@pytest.mark.parametrize('resident', ['1', '0'])
@pytest.mark.parametrize('ctrl', [False, True])
def test_trajnet_workspace_address_reused_by_other_shapes(ctrl, resident, monkeypatch):
    shapes = {'A': (9, 144), 'B': (1, 16), 'C': (9, 48)}
    run = lambda net, B, T: _traj_loop(net, resident, B, T) + _traj_forward(net, B, T)
    refs = {}
    for key, (B, T) in shapes.items():
        refs[key] = _run(lambda: run(_make_trajnet(ctrl), B, T), SM.ZEROS)
    net = _make_trajnet(ctrl)
    nbytes = max(_lib().rohm_trajnet_workspace_bytes(net.native(torch.device(DEV)).handle, B, T) for B, T in shapes.values())
    rec = _Recycler(nbytes, n=1)
    rec.install(monkeypatch)
    _sequence(rec, [(k, lambda k=k: run(net, *shapes[k])) for k in _ABAB], refs)
    assert rec.served == 6                                     # every change of shape drew the workspace again, from the arena


def test_gemm_res_layernorm_scratch_address_reused_by_the_other_shape(monkeypatch):
    shapes = {'A': (288, 512, 64), 'B': (144, 1024, 32)}
    refs = {k: _run(lambda: _gemm_res_layernorm(*s), SM.ZEROS) for k, s in shapes.items()}
    rec = _Recycler(max(_lib().rohm_gemm_res_layernorm_scratch_bytes(M, N) for M, N, _ in shapes.values()) + 64, n=1)
    rec.install(monkeypatch)
    _sequence(rec, [(k, lambda k=k: _gemm_res_layernorm(*shapes[k])) for k in 'ABABBAAB'], refs)
    assert rec.served == 8


def test_training_saved_and_scratch_addresses_reused_by_the_other_clip_length(monkeypatch):
    """T = 63 and T = 143 alternate in one `saved` and one `scratch` address (PoseNet), as a last partial batch does."""
    refs = {T: _run(lambda: _posenet_train(T, 0.1), SM.ZEROS) for T in (63, 143)}
    d = (512, 4, 1024, 1, 294, 272)
    nbytes = max(max(_lib().rohm_posenet_train_saved_bytes(*d, 2, T), _lib().rohm_posenet_train_scratch_bytes(*d, 2, T)) for T in (63, 143))
    rec = _Recycler(nbytes, n=2)
    rec.install(monkeypatch)
    _sequence(rec, [(T, lambda T=T: _posenet_train(T, 0.1)) for T in (143, 63, 143, 63, 63, 143)], refs)
    assert rec.served == 12


@pytest.mark.parametrize('chain', ['0', 'layer', 'stack'])
def test_posenet_module_alternating_batch_sizes(chain):
    """The cheap form through the module alone: net(B 3), net(B 1) x 40, net(B 3) -- the allocator usually hands the dropped workspace's
    block back -- against the first B = 3 result."""
    net = _make_posenet(chain)
    first = _pose_forward(net, 3, 143)
    one = _pose_forward(net, 1, 143)
    for _ in range(39):
        assert not SM.differences(_pose_forward(net, 1, 143), one)
    assert not SM.differences(_pose_forward(net, 3, 143), first)
    assert not SM.differences(_pose_loop(net, 3, 143), _pose_loop(_make_posenet(chain), 3, 143))
