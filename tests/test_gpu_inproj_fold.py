"""GPU: layer 0's in-projection folded onto the packed input (csrc/encoder_chain.hip gemm_phase FOLD, csrc/posenet.hip w_fold / tokq /
econdq).  In a sampling call of >= 4 steps that runs as stack launches, qkv0 = x_t . (Win0 . Wx)^T + (econd . Win0^T + bin0) replaces
h0 = x_t . Wx^T + econd; qkv0 = h0 . Win0^T + bin0 (model/posenet.py:85-92 up to the first encoder layer): a re-rounding of the same
quantity.  B = 25 is the smallest encoder_stack_kernel<8> launch in one part-filled round (forced with ROHM_POSENET_CHAIN_ANY=1: by
default such a batch runs one launch per GEMM), B = 48 the smallest <4> one.

Bars: 2e-5 against the same library with ROHM_POSENET_INPROJ_FOLD=0 (the project's bar for two roundings of one step sequence; a
torch-fp32 restatement of both forms differs by 3.5e-6 over 8 steps), 1e-4 against the float64 oracle (the bar of
tests/test_gpu_config_batches.py for a forward; the restatement is 3.3e-6 off float64).  The oracle runs three clips of the batch (first,
middle, last); every clip is compared folded against unfolded, and that difference must be non-zero (the folded form was taken)."""
import functools

import pytest
import torch

from helpers import cpu_noise_sequence, max_abs, seeded
from test_gpu_posenet import DEV, make_diffusion, make_posenet

pytestmark = pytest.mark.gpu

T = 143
IDX = [999, 0, 640, 311, 2, 1]      # chunk 4: a folded 4-step call that reads BOTH ends of tokq (rows 999 and 0; the loops take the
                                    # indices in any order), then a 2-step call on the unfolded phases (2, 1)
ORACLE_CLIPS = 3                    # the float64 oracle runs the first, a middle and the last clip only (clips are independent of each
                                    # other, and the folded-against-unfolded comparison covers every clip)


def _net(fold, seed=5):
    mp = pytest.MonkeyPatch()
    try:
        mp.setenv('ROHM_POSENET_CHAIN_ANY', '1')             # B = 25 runs launch per GEMM by default (part-filled round); both are
        if not fold:                                           # read when the handle is created
            mp.setenv('ROHM_POSENET_INPROJ_FOLD', '0')
        net, sd = make_posenet(seed)
        nat = net.native(torch.device(DEV))
    finally:
        mp.undo()
    if nat.exchange_mode & 32 == 0:
        pytest.skip(f'no encoder stack on this device: {nat.exchange_guard}')
    return net, sd


@functools.lru_cache(maxsize=None)
def _inputs(B):
    x_T, noises = cpu_noise_sequence(23, (B, 294, 1, T), len(IDX))
    return x_T, tuple(noises), seeded(24, B, 294, 1, T)


def _loop(net, B, profile=False):
    from rohm_amd import _lib
    x_T, noises, cond = _inputs(B)
    diff = make_diffusion(1000)
    diff.fused_chunk = 4
    diff._indices = lambda skip=0, early_stop=False: list(IDX)
    diff.noise_source = lambda step, like: (x_T if step == -1 else noises[step])
    if profile:
        _lib.profile_start(1)
    y = diff.p_sample_loop(net, {'cond': cond.to(DEV)}, [B, 294, 1, T])
    torch.cuda.synchronize()
    prof = _lib.profile_stop() if profile else None
    net.check_exchange()
    return y.clone(), prof


@functools.lru_cache(maxsize=None)
def _runs(B):
    """(folded result, its launch profile, unfolded result, its launch profile) of the 6-step loop, computed once per batch size."""
    on, _ = _net(True)
    off, _ = _net(False)
    y1, p1 = _loop(on, B, profile=True)
    y0, p0 = _loop(off, B, profile=True)
    return y1, p1, y0, p0


@pytest.mark.parametrize('B', [25, 48])
def test_folded_loop_matches_unfolded_and_oracle(B):
    from oracle import diffusion as odiff
    from oracle import nets
    y1, _, y0, _ = _runs(B)
    d = max_abs(y1, y0)
    x_T, noises, cond = _inputs(B)
    _, sd = make_posenet(5)
    clips = sorted({0, B // 2, B - 1})[:ORACLE_CLIPS]
    c64 = cond[clips]
    fn = lambda xx, i: nets.posenet_forward(sd, xx, c64, torch.full((len(clips),), i, dtype=torch.int64), dtype=torch.float64)
    ref = odiff.p_sample_loop(fn, x_T[clips], [n[clips] for n in noises], odiff.tables(odiff.cosine_betas(1000)), IDX, dtype=torch.float64)
    e = max_abs(y1[clips].cpu(), ref)
    print(f'B={B}: max|folded - unfolded| = {d:.3e}; max|folded - float64 oracle| = {e:.3e} (clips {clips}, |x| <= {float(ref.abs().max()):.2f})')
    assert torch.isfinite(y1).all()
    assert d > 0.0      # the folded form really ran: a re-rounding of qkv0 is not bit-equal to the unfolded phases
    assert d < 2e-5
    assert e < 1e-4


@pytest.mark.parametrize('B', [25, 48])
def test_folded_loop_is_bit_reproducible(B):
    y1 = _runs(B)[0]
    again, _ = _loop(_net(True)[0], B)
    assert torch.equal(again, y1)


@pytest.mark.parametrize('B', [25, 48])
def test_new_weights_rebuild_the_fold(B, monkeypatch):
    """load_state_dict on the same module (the supported route: the native handle follows the parameters' version counters): w_fold
    and tokq are rebuilt with the handle -- the result is a fresh module's, bit for bit."""
    from rohm_amd.utils import synth
    monkeypatch.setenv('ROHM_POSENET_CHAIN_ANY', '1')     # the handle is re-created inside the loop below: B = 25 must stack again
    net, _ = _net(True)
    _loop(net, B)                                          # the handle of seed 5 has run
    net.load_state_dict(synth.posenet_state_dict(6), strict=True)
    got, _ = _loop(net, B)
    want, _ = _loop(_net(True, seed=6)[0], B)
    assert torch.equal(got, want)
    assert not torch.equal(got, _runs(B)[0])


@pytest.mark.parametrize('B', [25, 48])
def test_one_more_launch_per_folded_call(B):
    """6 steps in chunks of 4: ONE folded call (4 steps) and one call too short to hoist (2 steps).  The fold costs exactly one
    launch per folded call (econdq), and every step stays one stack launch."""
    _, p1, _, p0 = _runs(B)
    n1, n0 = sum(v['launches'] for v in p1.values()), sum(v['launches'] for v in p0.values())
    print(f'B={B}: launches folded {n1} / unfolded {n0}:', {k: v['launches'] for k, v in p1.items()})
    assert p1['gemm_stack_tail']['launches'] == len(IDX) and p0['gemm_stack_tail']['launches'] == len(IDX)
    assert n1 == n0 + 1
    assert n1 <= len(IDX) + 4 * 2                          # the budget of tests/test_gpu_chain.py: steps + 4 per call


@pytest.mark.parametrize('B', [25, 48])
def test_workspace_one_byte_short_is_refused(B):
    import numpy as np
    from rohm_amd import _lib
    from rohm_amd._lib import lib, ptr, stream_ptr
    net, _ = _net(True)
    off, _ = _net(False)
    nat = net.native(torch.device(DEV))
    need = lib().rohm_posenet_workspace_bytes(nat.handle, B, T)
    assert need - lib().rohm_posenet_workspace_bytes(off.native(torch.device(DEV)).handle, B, T) >= B * 144 * 1536 * 4
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 256 == 0
    x = seeded(1, B, 294, 1, T).to(DEV)
    before = x.clone()
    cond = seeded(2, B, 294, 1, T).to(DEV)
    noise = seeded(3, 4, B, 294, 1, T).to(DEV)
    ts = np.asarray([9, 8, 7, 6], np.int64)
    coef = np.asarray([[0.05, 0.95, 0.1]] * 4, np.float32).reshape(-1)
    rc = lib().rohm_posenet_sample_loop(nat.handle, ptr(x), ptr(cond), ts.ctypes.data_as(_lib.c_int64_p), coef.ctypes.data_as(_lib.c_float_p),
                                        ptr(noise), None, None, 4, B, T, ptr(ws), need - 1, stream_ptr(x.device))
    torch.cuda.synchronize()
    assert rc == -3, rc                                    # ROHM_ERR_WORKSPACE (include/rohm_hip.h)
    assert torch.equal(x, before)                          # refused before any launch
    rc = lib().rohm_posenet_sample_loop(nat.handle, ptr(x), ptr(cond), ts.ctypes.data_as(_lib.c_int64_p), coef.ctypes.data_as(_lib.c_float_p),
                                        ptr(noise), None, None, 4, B, T, ptr(ws), need, stream_ptr(x.device))
    torch.cuda.synchronize()
    assert rc == 0 and torch.isfinite(x).all() and not torch.equal(x, before)
