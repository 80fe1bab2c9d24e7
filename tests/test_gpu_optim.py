"""GPU: rohm_amd.optim.AdamW (rohm_adamw_step, rohm_grad_norm) against torch.optim.AdamW.

The bar of every numeric comparison is optim_ref's: the native error against the float64 CPU run is at most 4 x the error of
torch's own float32 CPU run, per quantity (parameters, exp_avg, exp_avg_sq)."""
import copy
import ctypes as C

import pytest
import torch

import optim_ref as R
from rohm_amd import _lib, optim

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def native(max_grad_norm=None):
    return lambda groups: optim.AdamW(groups, max_grad_norm=max_grad_norm)


def assert_within_bar(res, r64, r32, what=''):
    own, bar = R.errors(res, r64), R.errors(r32, r64)
    print(what, 'native error', own, 'torch fp32 error', bar)
    for q in R.QUANTITIES:
        assert own[q] <= R.MARGIN * bar[q], (what, q, own[q], bar[q])


ULP = 2.0 ** -24      # only for the direct call below, whose reference is the formula written out, one step


@pytest.fixture(scope='module')
def parity():
    params, grads = R.make_inputs()
    r64, r32 = R.references(params, grads)
    return params, grads, r64, r32


def test_parity_with_torch_adamw(parity):
    params, grads, r64, r32 = parity
    ps, opt = R.run(native(), params, grads, torch.float32, DEV)
    assert_within_bar(R.results(ps, opt), r64, r32, 'parity')
    assert opt.last_grad_norm is None
    assert all(int(opt.state[p]['step']) == R.K and opt.state[p]['step'].device.type == 'cpu' for p in ps)


def _edge_case(shapes, steps=R.K):
    params, grads = R.make_inputs(shapes, steps, seed=3)
    r64, r32 = R.references(params, grads)
    ps, opt = R.run(native(), params, grads, torch.float32, DEV)
    return R.results(ps, opt), r64, r32


def test_one_more_tensor_than_a_launch_takes():
    per_launch, _ = optim.limits()
    assert per_launch >= 1
    res, r64, r32 = _edge_case([(1 + i % 5,) for i in range(per_launch + 1)])
    assert_within_bar(res, r64, r32, 'tensors_per_launch + 1')


def test_one_more_element_than_a_block_takes_and_a_0_dim_parameter():
    _, per_block = optim.limits()
    assert per_block >= 4
    res, r64, r32 = _edge_case([(per_block + 1,), (), (2 * per_block,), (per_block - 1,)])
    assert_within_bar(res, r64, r32, 'elems_per_block + 1')


GUARD = 64


def _layout(sizes, offsets):
    """Positions of tensors in one buffer: a 64-float guard band, then a tensor whose start is `offset` floats past a 16-byte
    boundary, and so on, closed by a guard band.  -> (starts, total length)."""
    starts, pos = [], 0
    for n, off in zip(sizes, offsets):
        pos += GUARD
        pos += (off - pos) % 4
        starts.append(pos)
        pos += n
    return starts, pos + GUARD


def test_views_into_a_shared_buffer_keep_their_guard_bands():
    """Parameters that start 1, 2 and 3 floats past a 16-byte boundary (gradients and state are aligned: the scalar path)."""
    _, per_block = optim.limits()
    sizes, offsets = [5, 67, per_block + 3, 130, 2 * per_block + 1, 9], [1, 2, 3, 0, 1, 3]
    starts, total = _layout(sizes, offsets)
    params, grads = R.make_inputs([(n,) for n in sizes], R.K, seed=4)
    r64, r32 = R.references(params, grads)
    sentinel = torch.randn(total, generator=torch.Generator().manual_seed(9))
    buf = sentinel.clone()
    for s, n, p in zip(starts, sizes, params):
        buf[s:s + n] = p
    buf = buf.to(DEV)
    assert buf.data_ptr() % 16 == 0
    ps = [buf[s:s + n].detach().requires_grad_() for s, n in zip(starts, sizes)]
    assert [p.data_ptr() % 16 // 4 for p in ps] == offsets
    opt = optim.AdamW(R.split_groups(ps))
    for row in grads:
        R.set_grads(ps, row)
        opt.step()
    assert_within_bar(R.results(ps, opt), r64, r32, 'views')
    after = buf.cpu()
    keep = torch.ones(total, dtype=torch.bool)
    for s, n in zip(starts, sizes):
        keep[s:s + n] = False
    assert torch.equal(after[keep].view(torch.int32), sentinel[keep].view(torch.int32))


@pytest.mark.parametrize('offset', [0, 1, 2, 3])
def test_the_vector_body_with_a_common_offset_keeps_its_guard_bands(offset):
    """rohm_adamw_step called directly with all four tensors `offset` floats past a 16-byte boundary (scalar head, 16-byte body,
    scalar tail), against the update written out in float64, next to its float32 evaluation."""
    _, per_block = optim.limits()
    sizes = [1, 2, 3, 4, 7, 8, per_block + 2, 2 * per_block + 5]
    starts, total = _layout(sizes, [offset] * len(sizes))
    g = torch.Generator().manual_seed(11 + offset)
    sent = [torch.randn(total, generator=g) for _ in range(4)]
    sent[3] = sent[3].abs()                                  # exp_avg_sq is not negative
    keep = torch.ones(total, dtype=torch.bool)
    for s, n in zip(starts, sizes):
        keep[s:s + n] = False
    bufs = [x.to(DEV) for x in sent]
    assert all(b.data_ptr() % 16 == 0 for b in bufs)
    views = [[b[s:s + n] for s, n in zip(starts, sizes)] for b in bufs]
    lr, b1, b2, eps, wd, step = 1e-3, 0.9, 0.999, 1e-8, 0.01, 5
    arrays = [(C.c_void_p * len(sizes))(*[v.data_ptr() for v in vs]) for vs in views]
    numel = (C.c_longlong * len(sizes))(*sizes)
    _lib.check(_lib.lib().rohm_adamw_step(*arrays, numel, len(sizes), lr, b1, b2, eps, wd, step, None, _lib.stream_ptr(DEV)),
               'rohm_adamw_step')
    torch.cuda.synchronize()
    after = [b.cpu() for b in bufs]

    def formula(dtype):
        p, gr, m, v = (x.to(dtype) for x in sent)
        p = p * (1 - lr * wd)
        m = m + (1 - b1) * (gr - m)
        v = v * b2 + (1 - b2) * gr * gr
        p = p - (lr / (1 - b1 ** step)) * m / (v.sqrt() / (1 - b2 ** step) ** 0.5 + eps)
        return p, m, v
    r64, r32 = formula(torch.float64), formula(torch.float32)
    for k, (i, name) in enumerate(((0, 'p'), (2, 'exp_avg'), (3, 'exp_avg_sq'))):
        inside = ~keep
        own = R.tensor_error(after[i][inside], r64[k][inside])
        bar = R.tensor_error(r32[k][inside], r64[k][inside])
        print(name, 'native', own, 'fp32 formula', bar)
        assert own <= R.MARGIN * max(bar, ULP), (name, own, bar)
    assert torch.equal(after[1], sent[1])                    # gradients are only read
    for i in (0, 2, 3):
        assert torch.equal(after[i][keep].view(torch.int32), sent[i][keep].view(torch.int32)), i


def test_a_parameter_without_a_gradient_is_left_alone():
    params, grads = R.make_inputs([(5,), (70,), (9,)], 2, seed=5)
    ps = [p.to(DEV).requires_grad_() for p in params]
    before = [p.detach().clone() for p in ps]
    opt = optim.AdamW(ps, lr=1e-2)
    for row in grads:
        R.set_grads(ps, row)
        ps[1].grad = None
        opt.step()
    assert torch.equal(ps[1].detach(), before[1]) and ps[1] not in opt.state and len(opt.state) == 2
    assert not torch.equal(ps[0].detach(), before[0]) and not torch.equal(ps[2].detach(), before[2])
    assert ps[1]._version == 0 and ps[0]._version >= 2


@pytest.mark.parametrize('first', ['native', 'torch'])
def test_state_moves_between_the_two_classes(parity, first):
    """3 steps of one class, state_dict() into the other, 3 more steps on each side: both continuations within the bar."""
    params, grads, _, _ = parity
    grads = grads[:6]
    r64, r32 = R.references(params, grads)
    make = {'native': native(), 'torch': R.torch_adamw()}
    other = 'torch' if first == 'native' else 'native'
    ps_a, opt_a = R.run(make[first], params, grads[:3], torch.float32, DEV)
    ps_b = [p.detach().clone().requires_grad_() for p in ps_a]
    opt_b = make[other](R.split_groups(ps_b))
    opt_b.load_state_dict(copy.deepcopy(opt_a.state_dict()))      # a live state_dict() shares its tensors with its optimiser
    assert [g['lr'] for g in opt_b.param_groups] == [g['lr'] for g in R.GROUPS]
    for ps, opt in ((ps_a, opt_a), (ps_b, opt_b)):
        for row in grads[3:]:
            R.set_grads(ps, row)
            opt.step()
        assert all(int(opt.state[p]['step']) == 6 for p in ps)
        assert_within_bar(R.results(ps, opt), r64, r32, f'{first} first, continued by {type(opt).__module__}')


def test_versions_advance_and_inference_sees_the_new_weights():
    import test_gpu_train_loop as TL
    from helpers import PoseDataset
    from rohm_amd.utils import synth
    B, T = 2, 15
    mean, std = synth.synthetic_stats(0)
    layer = TL._layer()
    net = TL._posenet(PoseDataset(mean, std), layer)
    g = torch.Generator().manual_seed(0)
    x, c, cot = (torch.randn(B, 294, 1, T, generator=g).to(DEV) for _ in range(3))
    t = torch.randint(0, 4, (B,), generator=g).to(DEV)
    batch = {'x_t': x, 'cond': c}
    net.eval()
    with torch.no_grad():
        stale = net(batch, t).clone()                      # the inference handle now caches the old weights
    net.train()
    trainable = [p for p in net.parameters() if p.requires_grad]
    opt = optim.AdamW(trainable, lr=1e-2, weight_decay=0.0)
    (net(batch, t) * cot).sum().backward()
    updated = [p for p in trainable if p.grad is not None]
    versions = [p._version for p in updated]
    opt.step()
    assert updated and all(p._version > v for p, v in zip(updated, versions))
    net.eval()
    with torch.no_grad():
        got = net(batch, t).clone()
    fresh = TL._posenet(PoseDataset(mean, std), layer)
    fresh.load_state_dict(net.state_dict(), strict=True)
    fresh.eval()
    with torch.no_grad():
        want = fresh(batch, t)
    assert not torch.equal(got, stale)
    assert torch.equal(got, want)


# ---- norm and clip -------------------------------------------------------------------------------------------------------------------
def _norm(opt_grads, max_norm):
    opt = optim.AdamW([g.clone().requires_grad_() for g in opt_grads], max_grad_norm=max_norm)
    coef = opt._grad_norm(opt_grads, [g.numel() for g in opt_grads], torch.device(DEV))
    assert coef.value == opt._norm_out.data_ptr() + 4
    return opt._norm_out.clone()


def test_total_norm_against_float64_and_bitwise_repeatable(parity):
    _, grads, _, _ = parity
    row = grads[0]
    exact = float(torch.sqrt(sum((g.double() ** 2).sum() for g in row)))
    ps = [g.clone().requires_grad_() for g in row]
    R.set_grads(ps, row)
    torch_norm = float(torch.nn.utils.clip_grad_norm_(ps, 1e30, foreach=False))
    torch_err = abs(torch_norm - exact) / exact
    dev = [g.to(DEV) for g in row]
    a, b = _norm(dev, 1.0), _norm(dev, 1.0)
    own_err = abs(float(a[0]) - exact) / exact
    print('native norm error', own_err, 'torch fp32 norm error', torch_err)
    assert own_err <= max(R.MARGIN * torch_err, 2.0 ** -22)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    want_coef = min(1.0, 1.0 / (exact + 1e-6))
    assert abs(float(a[1]) - want_coef) <= 2.0 ** -21 * want_coef
    assert float(_norm(dev, 2 * exact)[1]) == 1.0


def test_a_max_norm_above_the_norm_changes_no_bit(parity):
    params, grads, _, _ = parity
    ps0, opt0 = R.run(native(), params, grads[:3], torch.float32, DEV)
    ps1, opt1 = R.run(native(1e9), params, grads[:3], torch.float32, DEV)
    assert opt1.last_grad_norm is not None and opt1.last_grad_norm.is_cuda and opt1.last_grad_norm.dim() == 0
    a, b = R.results(ps0, opt0), R.results(ps1, opt1)
    for q in R.QUANTITIES:
        assert all(torch.equal(x, y) for x, y in zip(a[q], b[q])), q


def test_clipped_steps_against_float64_clip_then_adamw(parity):
    params, grads, _, _ = parity
    max_norm = 0.5                                         # the gradients' norm is about 1e3 x sqrt(5): well above
    r64, r32 = R.references(params, grads, max_norm=max_norm)
    ps, opt = R.run(native(max_norm), params, grads, torch.float32, DEV)
    assert float(opt.last_grad_norm) > 100 * max_norm
    assert_within_bar(R.results(ps, opt), r64, r32, 'clipped')
    # .grad itself is not rescaled
    assert all(torch.equal(p.grad.cpu(), g) for p, g in zip(ps, grads[-1]))
