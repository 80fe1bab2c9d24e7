"""The parity run of the native AdamW (rohm_amd/optim.py), shared by tests/test_gpu_optim.py and scripts/bench_optim.py --parity.

K steps on fixed seeded gradients, three ways: torch.optim.AdamW in float64 on the CPU (r64, foreach=False), the same in float32
(r32), and the optimiser under test.  The error of a tensor against r64 is  max |a - r64| / max(|r64|, 1e-3 max|r64|), taken
separately for parameters, exp_avg and exp_avg_sq as the maximum over all tensors.  The bar: at most MARGIN x r32's own error.
Both are fp32 evaluations of one formula that differ only in rounding (the device contracts to FMA), so they share an error
scale, not a value; a wrong formula (no bias correction, weight decay folded into the gradient, eps inside the root) lands
orders of magnitude away."""
import torch

SHAPES = [(), (1,), (3,), (5,), (63,), (64,), (65,), (10, 100), (4099,), (7, 10001)]
GROUPS = [dict(lr=1e-3, weight_decay=0.0), dict(lr=3e-4, weight_decay=0.01)]
K = 12
MARGIN = 4.0
QUANTITIES = ('p', 'exp_avg', 'exp_avg_sq')


def group_of(i):
    return i % len(GROUPS)


def make_inputs(shapes=SHAPES, steps=K, seed=0):
    """(params [n] float32, grads [steps][n] float32), on the CPU.  Gradient i is randn * 10^((i % 5) - 3); elements 1..3 of a
    tensor of >= 5 elements are 0, 1e-12 and 1e3."""
    g = torch.Generator().manual_seed(seed)
    params = [torch.randn(s, generator=g) for s in shapes]
    grads = []
    for _ in range(steps):
        row = []
        for i, s in enumerate(shapes):
            x = torch.randn(s, generator=g) * 10.0 ** ((i % 5) - 3)
            if x.numel() >= 5:
                flat = x.view(-1)
                flat[1], flat[2], flat[3] = 0.0, 1e-12, 1e3
            row.append(x)
        grads.append(row)
    return params, grads


def split_groups(tensors, groups=GROUPS):
    return [dict(params=[t for i, t in enumerate(tensors) if i % len(groups) == k], **g) for k, g in enumerate(groups)]


def set_grads(ps, row):
    for p, g in zip(ps, row):
        p.grad = g.to(dtype=p.dtype, device=p.device).clone()


def run(make_opt, params, grads, dtype, device, max_norm=None, clip_with_torch=False, groups=GROUPS):
    """Run len(grads) steps of make_opt(param groups) -> (ps, opt).  clip_with_torch: clip_grad_norm_(foreach=False) before every
    step (the torch references; the native optimiser clips inside its step)."""
    ps = [p.to(dtype=dtype, device=device).clone().requires_grad_() for p in params]
    opt = make_opt(split_groups(ps, groups))
    for row in grads:
        set_grads(ps, row)
        if clip_with_torch:
            torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False)
        opt.step()
    return ps, opt


def torch_adamw(**kw):
    return lambda groups: torch.optim.AdamW(groups, foreach=False, **kw)


def results(ps, opt):
    """{quantity: [tensor, ...]} as float64 CPU tensors; a parameter without state contributes None."""
    out = {q: [] for q in QUANTITIES}
    for p in ps:
        st = opt.state.get(p, {})
        out['p'].append(p.detach().double().cpu())
        for q in QUANTITIES[1:]:
            out[q].append(st[q].detach().double().cpu() if q in st else None)
    return out


def tensor_error(a, r64):
    scale = r64.abs().max()
    denom = torch.maximum(r64.abs(), 1e-3 * scale)
    diff = (a.double() - r64).abs()
    if scale == 0:
        return 0.0 if bool((diff == 0).all()) else float('inf')
    return float((diff / denom).max())


def errors(res, ref):
    """{quantity: max over tensors of tensor_error} of a results() dict against the float64 one."""
    return {q: max(tensor_error(a, r) for a, r in zip(res[q], ref[q]) if r is not None) for q in QUANTITIES}


def references(params, grads, max_norm=None, groups=GROUPS):
    """(r64 results, r32 results) of torch's CPU AdamW."""
    out = []
    for dtype in (torch.float64, torch.float32):
        ps, opt = run(torch_adamw(), params, grads, dtype, 'cpu', max_norm, clip_with_torch=max_norm is not None, groups=groups)
        out.append(results(ps, opt))
    return out
