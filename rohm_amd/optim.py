"""AdamW on the native library: `rohm_adamw_step` (one fused multi-tensor pass) and `rohm_grad_norm` (a bitwise reproducible
global gradient norm and the clip coefficient, never read on the host).

`AdamW` is a `torch.optim.Optimizer`: param groups with their own lr / betas / eps / weight_decay, torch's per-parameter state
(`step`, `exp_avg`, `exp_avg_sq`, created at a parameter's first step; a parameter without a gradient is skipped and gets none),
and a `state_dict()` that loads into `torch.optim.AdamW` and back.  The update is torch's `_single_tensor_adam` in fp32, operation
for operation; the device contracts multiply-adds, so results agree with torch's to rounding, not bitwise.

`max_grad_norm`: the global L2 norm over every gradient of the step (all groups, as `torch.nn.utils.clip_grad_norm_` over all
parameters) is computed on the device and the update multiplies each gradient by min(1, max_grad_norm / (norm + 1e-6)) as it reads
it.  Unlike `clip_grad_norm_`, `.grad` itself is NOT rescaled.  `last_grad_norm` is the norm as a device scalar; nothing reads it
on the host unless the caller does.  A non-finite norm behaves as torch's with `error_if_nonfinite=False`.

The group options `foreach` and `fused` (torch's keys, kept so that state dicts interchange) choose among torch's own
implementations and are ignored here: the step is always the one fused multi-tensor pass.  `state_dict()` hands out copies of
the host step counters (inside, the counters of the parameters that step together are views of one host tensor, and torch's
`load_state_dict` keeps a host `step` tensor as it is, so a live native state dict would otherwise share them with its loader).

`step()` raises while the current stream records a graph: the step count is a host scalar of `rohm_adamw_step`, and a graph would
repeat the recorded count -- its bias correction -- at every replay while the counters here stand still (torch's non-capturable
AdamW raises there too).  The entry point itself records (include/rohm_hip.h, "recordable calls").

There is no eager fallback: parameters must be contiguous fp32 tensors on a HIP device with dense gradients.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

_REFUSED = ('amsgrad', 'maximize', 'capturable', 'differentiable')


def limits():
    """(tensors per launch, elements per block) of rohm_adamw_step."""
    n, e = C.c_int(0), C.c_int(0)
    _lib.check(_lib.lib().rohm_adamw_limits(C.byref(n), C.byref(e)), 'rohm_adamw_limits')
    return n.value, e.value


def _pointers(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


class AdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None, *, amsgrad=False,
                 maximize=False, capturable=False, differentiable=False):
        for name, value in (('amsgrad', amsgrad), ('maximize', maximize), ('capturable', capturable),
                            ('differentiable', differentiable)):
            if value:
                raise ValueError(f'rohm_amd.optim.AdamW does not support {name}=True')
        if isinstance(lr, torch.Tensor) or any(isinstance(b, torch.Tensor) for b in betas):
            raise ValueError('rohm_amd.optim.AdamW takes lr and betas as Python floats')
        if not 0.0 <= lr:
            raise ValueError(f'Invalid learning rate: {lr}')
        if not 0.0 <= eps:
            raise ValueError(f'Invalid epsilon value: {eps}')
        if not 0.5 < betas[0] < 1.0:
            raise ValueError(f'Invalid beta parameter at index 0: {betas[0]} (the native step takes 0.5 < beta1 < 1)')
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f'Invalid beta parameter at index 1: {betas[1]}')
        if not 0.0 <= weight_decay:
            raise ValueError(f'Invalid weight_decay value: {weight_decay}')
        if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:
            raise ValueError(f'Invalid max_grad_norm: {max_grad_norm}')
        # torch's own group keys, so that a state_dict moves between the two classes in both directions
        defaults = dict(torch.optim.AdamW([torch.zeros(1)], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay).defaults)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.last_grad_norm = None
        self._norm_out = self._norm_scratch = self._step_buf = None
        self._step_views = []
        super().__init__(params, defaults)

    @staticmethod
    def _check_param(p):
        if p.dtype != torch.float32:
            raise ValueError(f'rohm_amd.optim.AdamW takes fp32 parameters, got {p.dtype}')
        if not p.is_cuda:
            raise ValueError('rohm_amd.optim.AdamW takes parameters on a HIP device (there is no CPU fallback)')
        if not p.is_contiguous():
            raise ValueError('rohm_amd.optim.AdamW takes contiguous parameters')

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        for p in self.param_groups[-1]['params']:
            self._check_param(p)
            if getattr(self, '_device', None) is None:
                self._device = p.device
            elif p.device != self._device:
                raise ValueError('rohm_amd.optim.AdamW: all parameters must be on one device')

    def state_dict(self):
        out = super().state_dict()
        out['state'] = {k: ({**st, 'step': st['step'].clone()} if isinstance(st.get('step'), torch.Tensor) else st)
                        for k, st in out['state'].items()}
        return out

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            self._check_group(group)
        for p, state in self.state.items():
            for key in ('exp_avg', 'exp_avg_sq'):
                s = state.get(key)
                if s is None or s.dtype != torch.float32 or s.device != p.device or s.shape != p.shape or not s.is_contiguous():
                    raise RuntimeError(f'rohm_amd.optim.AdamW: loaded state {key!r} does not match its parameter (fp32, same '
                                       'device, same shape, contiguous)')
            if 'step' not in state:
                raise RuntimeError("rohm_amd.optim.AdamW: loaded state has no 'step'")

    def _check_group(self, group):
        for name in _REFUSED:
            if group.get(name):
                raise RuntimeError(f'rohm_amd.optim.AdamW does not support {name}=True (param group option)')
        if group.get('decoupled_weight_decay') is False:
            raise RuntimeError('rohm_amd.optim.AdamW is AdamW: decoupled_weight_decay=False is not supported')

    def _state_of(self, p):
        """The parameter's state, created at its first step (what is loaded is checked in load_state_dict)."""
        state = self.state[p]
        if len(state) == 0:
            state['step'] = torch.tensor(0.0, dtype=torch.float32)      # on the host, as torch keeps it
            state['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return state

    def _grad_norm(self, grads, numel, device):
        """rohm_grad_norm over `grads` -> the device pointer of the clip coefficient."""
        lib = _lib.lib()
        need = lib.rohm_grad_norm_scratch_bytes(sum(numel), len(grads))
        if self._norm_out is None or self._norm_out.device != device:
            self._norm_out = torch.zeros(2, dtype=torch.float32, device=device)
            self._norm_scratch = None
        if self._norm_scratch is None or self._norm_scratch.numel() * 8 < need:
            self._norm_scratch = torch.empty((need + 7) // 8, dtype=torch.float64, device=device)
        _lib.check(lib.rohm_grad_norm(_pointers(grads), (C.c_longlong * len(numel))(*numel), len(grads), self.max_grad_norm,
                                      _lib.ptr(self._norm_out), _lib.ptr(self._norm_scratch), self._norm_scratch.numel() * 8,
                                      _lib.stream_ptr(device)), 'rohm_grad_norm')
        self.last_grad_norm = self._norm_out[0]
        return C.c_void_p(self._norm_out.data_ptr() + 4)

    def _advance(self, states):
        """step += 1 in every state -> the new values.  A 0-dim host tensor costs microseconds to add to, more than the rest of
        the host side per parameter, so the counters of the parameters that step together are kept as views of ONE host tensor:
        one add and one read serve them all.  Counters that are not yet such views (new, loaded, or the set changed) are
        advanced one by one and then moved into a fresh shared tensor; they stay 0-dim fp32 tensors in `state`, as torch's."""
        steps = [st['step'] for st in states]
        views = self._step_views
        if len(steps) == len(views) and all(a is b for a, b in zip(steps, views)):
            self._step_buf.add_(1)
            return self._step_buf.tolist()
        values = [float(s.add_(1).item()) for s in steps]
        self._step_buf = torch.tensor(values, dtype=torch.float32)
        self._step_views = list(self._step_buf.unbind(0))
        for st, view in zip(states, self._step_views):
            st['step'] = view
        return values

    def _refuse_while_recording(self):
        """Raise while the current stream records a graph, before the closure runs, any state is created or anything is issued: the
        step count is a host scalar of rohm_adamw_step, a graph would hold this call's value, and every replay would repeat its bias
        correction while the counters here stand still (torch's non-capturable AdamW raises there too)."""
        device = getattr(self, '_device', None)
        if device is None:
            return
        with torch.cuda.device(device):
            if not torch.cuda.is_current_stream_capturing():
                return
        counts = [int(st['step']) for st in self.state.values() if 'step' in st]      # (read only: no state is created here)
        raise RuntimeError(f'rohm_amd.optim.AdamW.step() cannot be recorded into a graph: the step count is a host scalar, and every '
                           f'replay would repeat the frozen step count {max(counts, default=0) + 1}.  Step outside the capture, or '
                           f'record rohm_adamw_step yourself with the step you mean to replay.')

    @torch.no_grad()
    def step(self, closure=None):
        self._refuse_while_recording()
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        # The host side is a large part of a step over a few hundred small tensors: per parameter only what can change between
        # steps is looked at (the gradient); parameters were checked when their group was added, state when it was made or loaded.
        f32, strided = torch.float32, torch.strided
        runs, all_grads, all_numel, states = [], [], [], []
        for group in self.param_groups:
            self._check_group(group)
            ps, gs, ms, vs, numel = [], [], [], [], []
            for p in group['params']:
                g = p.grad
                if g is None:
                    continue
                if g.layout is not strided:
                    raise RuntimeError('rohm_amd.optim.AdamW does not support sparse gradients')
                n = p.numel()
                if g.dtype is not f32 or not g.is_cuda or g.numel() != n or not p.is_contiguous():
                    raise RuntimeError('rohm_amd.optim.AdamW: parameters must be contiguous, gradients fp32, on the device and of '
                                       'their parameter\'s size')
                if not g.is_contiguous():
                    g = g.contiguous()
                state = self.state[p]
                if not state:
                    state = self._state_of(p)
                ps.append(p)
                gs.append(g)
                ms.append(state['exp_avg'])
                vs.append(state['exp_avg_sq'])
                states.append(state)
                numel.append(n)
            if ps:
                runs.append((group, ps, gs, ms, vs, numel))
                all_grads += gs
                all_numel += numel
        if not runs:
            return loss
        values, first, by_value = self._advance(states), 0, []
        for group, ps, gs, ms, vs, numel in runs:
            mine = values[first:first + len(ps)]
            first += len(ps)
            if mine.count(mine[0]) == len(mine):
                by_value.append((group, int(mine[0]), ps, gs, ms, vs, numel))
            else:                            # one sequence per step value
                for value in sorted(set(mine)):
                    pick = [i for i, x in enumerate(mine) if x == value]
                    by_value.append((group, int(value)) + tuple([lst[i] for i in pick] for lst in (ps, gs, ms, vs, numel)))
        lib, device = _lib.lib(), self._device
        with torch.cuda.device(device):
            coef = self._grad_norm(all_grads, all_numel, device) if self.max_grad_norm is not None else None
            stream = _lib.stream_ptr(device)
            for group, step, ps, gs, ms, vs, numel in by_value:
                beta1, beta2 = group['betas']
                _lib.check(lib.rohm_adamw_step(_pointers(ps), _pointers(gs), _pointers(ms), _pointers(vs),
                                               (C.c_longlong * len(numel))(*numel), len(ps), float(group['lr']), float(beta1),
                                               float(beta2), float(group['eps']), float(group['weight_decay']), step, coef, stream),
                           'rohm_adamw_step')
                # the kernel wrote behind autograd's back: move the version counters, which key the models' cached inference handles
                torch.autograd.graph.increment_version(ps)
        return loss
