"""GPU: the stack's staging addresses as a scalar base plus a 32-bit lane offset (csrc/encoder_chain.hip stage_rsrc / stage_lane_off).

A six-step sampling loop through rohm_posenet_sample_loop -- one call of 4 steps (it hoists: the folded in-projection) and one of 2
(under 4 steps: the unfolded leading phases) -- at B = 48 (encoder_stack_kernel<4> in a part-filled round of 192 workgroups: the
smallest batch that runs the 4-part code with its head-aligned tiles and resident attention) and B = 32 (encoder_stack_kernel<8>):

  * the stack against the same weights with ROHM_POSENET_CHAIN=0 (one launch per GEMM), inside the project's bar of 2e-5 for two
    roundings of one step sequence, and two runs of the stack bit-equal;
  * the same loop with x, cond and the noise as views at an element offset of 3 (4-byte aligned, not 16-byte aligned) into larger
    allocations, and the workspace allocated behind a filler of more than 2^31 bytes: bases and offsets the default allocator does not
    produce.  Where the arrays live must not change a bit of the result, and the bar against ROHM_POSENET_CHAIN=0 is the same.

Every run's inputs are the same seeded arrays; the launch-per-GEMM reference is computed once per batch size."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from helpers import max_abs, seeded
from test_gpu_posenet import DEV, make_posenet

pytestmark = pytest.mark.gpu

T = 143
TS = [999, 0, 640, 311, 2, 1]
CALLS = [(0, 4), (4, 6)]
COEF = [[0.05, 0.95, 0.1]] * len(TS)       # (coef1, coef2, sigma): x stays of order 1 over the six steps
BAR = 2e-5
FILLER_BYTES = (1 << 31) + (3 << 20) + 256


def _net(stack):
    mp = pytest.MonkeyPatch()
    try:
        if not stack:
            mp.setenv('ROHM_POSENET_CHAIN', '0')      # read when the handle is created
        net, _ = make_posenet(5)
        nat = net.native(torch.device(DEV))
    finally:
        mp.undo()
    if stack and nat.exchange_mode & 32 == 0:
        pytest.skip(f'no encoder stack on this device: {nat.exchange_guard}')
    assert stack or nat.exchange_mode & 48 == 0
    return net


@functools.lru_cache(maxsize=None)
def _inputs(B):
    return seeded(31, B, 294, 1, T), seeded(32, B, 294, 1, T), seeded(33, len(TS), B, 294, 1, T)


def _place(src, offset):
    """a device copy of `src`: its own allocation, or a view `offset` elements into a larger one"""
    if offset == 0:
        return src.to(DEV), None
    big = torch.empty(src.numel() + offset + 5, dtype=torch.float32, device=DEV)
    view = big[offset:offset + src.numel()].view(src.shape)
    view.copy_(src)
    assert view.is_contiguous() and view.data_ptr() % 16 == (4 * offset) % 16
    return view, big


def _loop(net, B, offset=0, filler=False):
    from rohm_amd import _lib
    from rohm_amd._lib import lib, ptr, stream_ptr
    nat = net.native(torch.device(DEV))
    x0, cond0, noise0 = _inputs(B)
    keep = [torch.empty(FILLER_BYTES, dtype=torch.uint8, device=DEV)] if filler else []
    need = lib().rohm_posenet_workspace_bytes(nat.handle, B, T)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 256 == 0
    (x, kx), (cond, kc), (noise, kn) = _place(x0, offset), _place(cond0, offset), _place(noise0, offset)
    keep += [kx, kc, kn]
    coef = np.asarray(COEF, np.float32)
    per_step = x0.numel()
    for lo, hi in CALLS:
        ts = np.asarray(TS[lo:hi], np.int64)
        cf = np.ascontiguousarray(coef[lo:hi]).reshape(-1)
        nz = noise.view(-1)[lo * per_step:hi * per_step].view(hi - lo, *x0.shape)
        rc = lib().rohm_posenet_sample_loop(nat.handle, ptr(x), ptr(cond), ts.ctypes.data_as(_lib.c_int64_p), cf.ctypes.data_as(_lib.c_float_p),
                                            ptr(nz), None, None, hi - lo, B, T, ptr(ws), need, stream_ptr(x.device))
        assert rc == 0, (rc, lib().rohm_last_error())
        rc = lib().rohm_posenet_exchange_status(nat.handle, B, T, ptr(ws), need, stream_ptr(x.device))
        assert rc == 0, (rc, lib().rohm_last_error())
    torch.cuda.synchronize()
    out = x.clone()
    del keep
    return out


@functools.lru_cache(maxsize=None)
def _reference(B):
    """the six steps with one launch per GEMM, once per batch size"""
    return _loop(_net(False), B)


@functools.lru_cache(maxsize=None)
def _stack(B):
    return _loop(_net(True), B)


@pytest.mark.parametrize('B', [48, 32])
def test_stack_loop_matches_launch_per_gemm(B):
    y, ref = _stack(B), _reference(B)
    d = max_abs(y, ref)
    print(f'B={B}: max|stack - launch per GEMM| = {d:.3e} (|x| <= {float(ref.abs().max()):.2f})')
    assert torch.isfinite(y).all()
    assert d > 0.0          # the other form really ran
    assert d < BAR


@pytest.mark.parametrize('B', [48, 32])
def test_stack_loop_is_bit_reproducible(B):
    assert torch.equal(_loop(_net(True), B), _stack(B))


@pytest.mark.parametrize('B', [48, 32])
def test_stack_loop_on_offset_views_behind_a_filler(B):
    y = _loop(_net(True), B, offset=3, filler=True)
    ref = _reference(B)
    d = max_abs(y, ref)
    print(f'B={B}: offset views, workspace behind {FILLER_BYTES} bytes: max|stack - launch per GEMM| = {d:.3e}')
    assert torch.isfinite(y).all()
    assert d < BAR
    assert torch.equal(y, _stack(B))      # where the arrays live changes no bit
