"""GPU: the three building blocks of the C ABI (rohm_gemm_f32, rohm_layernorm_f32, rohm_attention_f32) at ragged, strided and
unaligned edges, every operand carved out of a guarded canvas.

Each operand is a view into a larger flat device buffer with at least one tile (144 rows) of slack before and after it.  Input padding
is NaN -- a value read from outside the operand poisons the result -- and output canvases hold a sentinel: after the launch everything
outside the M x N window must be bit-identical (compared as int32) to a copy taken before it, and the window must be finite and within
the project's own error bar of a float64 CPU evaluation of the same operation (the bars of test_gpu_kernels.py).

Worst errors seen on an MI355X (max abs against float64; `pytest -s` prints them as they come):
    GEMM (a) tails on the 64-wide tile      2.1e-6                                      bar 2e-5 sqrt(K / 32)
    GEMM (b) one disqualifier at a time     1.2e-6                                      bar 2.8e-5
    GEMM (c) wide tiles, ragged             1.7e-6 / 2.5e-6 / 2.5e-6 / 5.3e-6           bar 2e-5 / 2.8e-5 / 3.5e-5 / 8e-5
                                            at K = 32 / 64 / 96 / 512
    LayerNorm (e)                           1.8e-6; rows of mean 600: 1.9e-4            bar 5e-6; 5e-4
    attention (f)                           general 1.1e-6, specialised 1.3e-6          bar 5e-6

What the guard bands can and cannot see: a store outside the window changes bits and fails the comparison; a load outside an operand
is seen only if the value reaches the result (a padding NaN in the window).  A value read from the padding and then dropped, such as
the bias of a column that is never stored, leaves no trace here.
"""
import functools
import math

import pytest
import torch

from helpers import seeded
from oracle import nets

pytestmark = pytest.mark.gpu

TILE = 144               # rows of slack on either side of every operand (the GEMM's row tile, the attention's clip)
SENTINEL = 7.5
NAN = float('nan')
WORST = {}               # family -> worst error so far (printed by every test that updates it)


def _dev():
    return torch.device('cuda', 0)


def _note(family, err):
    WORST[family] = max(WORST.get(family, 0.0), err)
    print(f'{family}: {err:.3e} (worst so far {WORST[family]:.3e})')


class Canvas:
    """A [rows, cols] operand inside a flat device buffer: `ld` floats from row to row, the first element `shift` floats behind a
    16-byte boundary, 144 * ld floats of slack in front of it and behind it, everything that is not the operand = `fill`."""

    def __init__(self, rows, cols, ld=None, shift=0, fill=NAN, data=None):
        ld = cols if ld is None else ld
        slack = TILE * max(ld, cols)                       # a multiple of 4 floats: the operand's alignment is `shift` alone
        self.shape, self.strides, self.off = (rows, cols), (ld, 1), slack + shift
        self.flat = torch.full((slack + shift + rows * max(ld, cols) + slack,), fill, device=_dev(), dtype=torch.float32)
        self.view = torch.as_strided(self.flat, self.shape, self.strides, self.off)
        assert self.flat.data_ptr() % 16 == 0 and (self.view.data_ptr() % 16 == 0) == (shift % 4 == 0)
        if data is not None:
            self.view.copy_(data.to(_dev()))
        self.before = self.flat.clone()

    def untouched(self):
        """Every bit of the buffer, the operand included, as it was before the launch."""
        return torch.equal(self.flat.view(torch.int32), self.before.view(torch.int32))

    def outside_untouched(self):
        """Every bit of the buffer outside the operand's window as it was before the launch."""
        after = self.flat.clone()
        torch.as_strided(after, self.shape, self.strides, self.off).copy_(torch.as_strided(self.before, self.shape, self.strides, self.off))
        return torch.equal(after.view(torch.int32), self.before.view(torch.int32))


def _vec(data, shift=0):
    """A vector operand (bias, gamma, beta) in a canvas of its own -> (canvas, 1-D view)."""
    c = Canvas(1, data.numel(), shift=shift, data=data[None])
    return c, c.view[0]


def _window_error(win, ref):
    """(max abs error of the window against the float64 reference, all finite?) -- the subtraction runs in float64 on the device."""
    r = ref.to(_dev())
    return float((win.double() - r).abs().max()), bool(torch.isfinite(win).all())


# ------------------------------------------------------------------------------------------------------------------ GEMM
def _gemm_ref(a, w, bias, res, epi):
    r = a.double() @ w.double().T
    if bias is not None:
        r = r + bias.double()
    if epi == 1:
        r = nets.gelu_erf(r)
    if epi == 2:
        r = r + res.double()
    return r


def _gemm_bar(K):
    return 2e-5 * math.sqrt(K / 32)


def _gemm_launch(a, w, bias, res, epi, ref, lda=None, ldw=None, ldc=None, ldr=None, c_shift=0, bias_shift=0, r_shift=0):
    """One launch on canvases; asserts the guard bands, returns (error of the window, the GEMM's profiler label)."""
    from rohm_amd import _lib, ops
    (M, K), N = a.shape, w.shape[0]
    A, W = Canvas(M, K, ld=lda, data=a), Canvas(N, K, ld=ldw, data=w)
    B, bias_v = _vec(bias, bias_shift) if bias is not None else (None, None)
    R = Canvas(M, N, ld=ldr, shift=r_shift, data=res) if res is not None else None
    C = Canvas(M, N, ld=ldc, shift=c_shift, fill=SENTINEL)
    _lib.profile_start(1)
    try:
        out = ops.gemm(A.view, W.view, bias_v, R.view if R is not None else None, epi, out=C.view)
    finally:
        rows = _lib.profile_stop()
    labels = [k for k in rows if k.startswith('gemm_')]
    assert len(labels) == 1 and rows[labels[0]]['launches'] == 1, rows
    assert labels[0].split('/')[0] == ('gemm_bias', 'gemm_bias_gelu', 'gemm_bias_res')[epi], labels
    assert out.data_ptr() == C.view.data_ptr()
    err, finite = _window_error(C.view, ref)
    assert C.outside_untouched(), 'the kernel wrote outside its M x N window'
    assert all(c.untouched() for c in (A, W, B, R) if c is not None), 'the kernel wrote to an input operand'
    assert finite, 'non-finite output: padding was read into the result'
    assert err < _gemm_bar(K), (err, _gemm_bar(K))
    return err, labels[0]


@functools.lru_cache(maxsize=4)
def _small_inputs(M, N, K):
    """Drawn as test_gpu_kernels.py::test_gemm draws them."""
    return seeded(M + N, M, K), seeded(K + 7, N, K) / math.sqrt(K), seeded(3, N), seeded(4, M, N)


def _tail_cases():
    """(a): the 35 (M, N) pairs, K and (epi, bias?) cycling underneath so that every value of every axis appears at least twice and
    every (epi, bias?) pair meets K = 32 and K = 96 (twice each: pair index i // 3 runs over 0..11 on each residue of i mod 3)."""
    Ms, Ns, Ks = (1, 17, 143, 145, 289), (1, 3, 4, 5, 63, 65, 130), (32, 96, 160)
    pairs = [(e, b) for e in (0, 1, 2) for b in (True, False)]
    cases = []
    for i, (M, N) in enumerate((M, N) for M in Ms for N in Ns):
        cases.append((M, N, Ks[i % 3]) + pairs[(i // 3) % 6])
    for ax, vals in enumerate((Ms, Ns, Ks)):
        assert all(sum(c[ax] == v for c in cases) >= 2 for v in vals)
    for K in (32, 96):
        assert {c[3:] for c in cases if c[2] == K} == set(pairs)
    assert len(cases) <= 60
    return cases


@pytest.mark.parametrize('M,N,K,epi,with_bias', _tail_cases())
def test_gemm_tails_on_the_64_wide_tile(M, N, K, epi, with_bias):
    """(a) Row and column tails of the 144 x 64 tile, a single K chunk (no second prologue DMA) and odd chunk counts (the other
    double-buffer parity at loop exit), with and without bias.  N = 4 takes the guarded vector store, every other N the scalar one."""
    a, w, bias, res = _small_inputs(M, N, K)
    bias = bias if with_bias else None
    err, label = _gemm_launch(a, w, bias, res if epi == 2 else None, epi, _gemm_ref(a, w, bias, res, epi))
    assert label.endswith('/64'), label
    _note('gemm (a) tails', err)


# (b): M = 144, N = 128, K = 64 with aligned, contiguous operands and a bias takes the FULL instantiation (no edge masks, 16-byte
# accesses only); each variation changes ONE operand.  The residual is passed with every epilogue: only epilogue 2 may look at it.
_DISQUALIFIERS = {
    'ldc=N+4 (stays FULL)': dict(ldc=128 + 4),
    'ldc=N+1': dict(ldc=128 + 1),
    'C+1': dict(c_shift=1),
    'bias+1': dict(bias_shift=1),
    'bias=None': dict(no_bias=True),
    'R+1': dict(r_shift=1),
    'ldr=N+1': dict(ldr=128 + 1),
    'ldr=N+4': dict(ldr=128 + 4),
    'lda=K+4': dict(lda=64 + 4),
    'ldw=K+8': dict(ldw=64 + 8),
}


@pytest.mark.parametrize('epi', [0, 1, 2])
@pytest.mark.parametrize('what', list(_DISQUALIFIERS))
def test_gemm_one_disqualifier_at_a_time(what, epi):
    a, w, bias, res = _small_inputs(144, 128, 64)
    kw = dict(_DISQUALIFIERS[what])
    if kw.pop('no_bias', False):
        bias = None
    err, _ = _gemm_launch(a, w, bias, res, epi, _gemm_ref(a, w, bias, res, epi), **kw)
    _note('gemm (b) disqualifiers', err)


# (c): with N = 1536 the launcher's cost rule (rounds of 256 workgroups x (tile width + 24)) picks the tile width from the number of
# 144-row tiles alone:
#       row tiles   width
#          11        128
#          22        192
#          33        256
#          43        384
# The profiler label only tells the 64-wide tile ("/64") from the wide ones, so the table is documented here, not re-derived.
_WIDE_N = 1536
_WIDE_TM = {128: 11, 192: 22, 256: 33, 384: 43}
_WIDE_ROWS = TILE * max(_WIDE_TM.values())
LABELS_SEEN = set()


@functools.lru_cache(maxsize=1)
def _wide_res():
    return seeded(4, _WIDE_ROWS, _WIDE_N)


@functools.lru_cache(maxsize=2)
def _wide_inputs(K):
    """One draw for all widths: a problem of tm row tiles uses the first rows of A and R.  -> a, w, bias, a @ w^T in float64."""
    a, w = seeded(_WIDE_ROWS + _WIDE_N, _WIDE_ROWS, K), seeded(K + 7, _WIDE_N, K) / math.sqrt(K)
    return a, w, seeded(3, _WIDE_N), a.double() @ w.double().T


@functools.lru_cache(maxsize=2)
def _wide_ref(K, epi, with_bias):
    """The float64 result of all _WIDE_ROWS rows (row m depends on row m of A and R only: a smaller problem is a row slice)."""
    _, _, bias, r = _wide_inputs(K)
    if with_bias:
        r = r + bias.double()
    if epi == 1:
        r = nets.gelu_erf(r)
    if epi == 2:
        r = r + _wide_res().double()
    return r


def _wide_launch(M, K, epi, with_bias=True, **kw):
    a, w, bias, _ = _wide_inputs(K)
    err, label = _gemm_launch(a[:M], w, bias if with_bias else None, _wide_res()[:M] if epi == 2 else None, epi,
                              _wide_ref(K, epi, with_bias)[:M], **kw)
    LABELS_SEEN.add(label)
    assert '/64' not in label, f'{label}: the 64-wide tile ran, not a wide one'
    return err


@pytest.mark.parametrize('epi,width', [(e, bn) for e in (0, 1, 2) for bn in _WIDE_TM])      # (the order keeps _wide_ref's cache warm)
def test_gemm_wide_tiles_ragged(epi, width):
    """gemm_f32_kernel<128 | 192 | 256 | 384, epi, FULL = false>: the guarded epilogue (bias, residual and store, each in its vector
    and its scalar form) of the wide tiles, and their FULL form on strided C / R."""
    tm, N = _WIDE_TM[width], _WIDE_N
    errs = [_wide_launch(TILE * tm - 5, 64, epi),                                   # partial last row tile
            _wide_launch(TILE * tm, 64, epi, with_bias=False),
            _wide_launch(TILE * tm, 64, epi, bias_shift=1),
            _wide_launch(TILE * tm, 64, epi, ldc=N + 1)]                            # scalar stores
    if epi == 2:
        errs.append(_wide_launch(TILE * tm, 64, epi, ldr=N + 1))                    # scalar residual loads, vector stores
    errs.append(_wide_launch(TILE * tm, 64, epi, ldc=N + 4, ldr=N + 8 if epi == 2 else None))      # FULL
    _note('gemm (c) wide tiles K=64', max(errs))
    print('labels seen:', sorted(LABELS_SEEN))


@pytest.mark.parametrize('K,width,epi', [(512, 128, 2), (512, 192, 1), (512, 256, 0), (512, 384, 2),
                                         (32, 128, 0), (32, 192, 2), (32, 256, 1), (32, 384, 0),
                                         (96, 128, 1), (96, 192, 0), (96, 256, 2), (96, 384, 1)])
def test_gemm_wide_tiles_ragged_other_depths(K, width, epi):
    """The same instantiations over 16 K chunks, over a single one (the peeled last iteration is the only one; the 384-wide tile,
    whose loop is not peeled, re-fetches its only chunk) and over three (odd: the other buffer at loop exit)."""
    _note(f'gemm (c) wide tiles K={K}', _wide_launch(TILE * _WIDE_TM[width] - 5, K, epi))
    print('labels seen:', sorted(LABELS_SEEN))


_REFUSALS = {
    'K=48': (dict(K=48), 'K=48'),
    'lda=K+2': (dict(lda=64 + 2), 'lda'),
    'A+1': (dict(a_shift=1), 'aligned'),
    'lda<K': (dict(lda=64 - 4), 'lda=60'),
    'ldw<K': (dict(ldw=64 - 4), 'ldw=60'),
    'ldc<N': (dict(ldc=128 - 4), 'ldc=124'),
    'ldr<N': (dict(ldr=128 - 4), 'ldr=124'),
}


@pytest.mark.parametrize('what', list(_REFUSALS))
def test_gemm_refusals(what):
    """(d) What rohm_gemm_f32 cannot run it refuses, naming the argument, before anything is launched: C keeps its bits."""
    from rohm_amd import _lib, ops
    kw, word = _REFUSALS[what]
    M, N, K = 144, 128, kw.get('K', 64)
    A = Canvas(M, K, ld=kw.get('lda'), shift=kw.get('a_shift', 0), fill=0.0)
    W, R = Canvas(N, K, ld=kw.get('ldw'), fill=0.0), Canvas(M, N, ld=kw.get('ldr'), fill=0.0)
    B, bias_v = _vec(torch.zeros(N))
    C = Canvas(M, N, ld=kw.get('ldc'), fill=SENTINEL)
    with pytest.raises(_lib.RohmHipError, match=word):
        ops.gemm(A.view, W.view, bias_v, R.view, 2, out=C.view)
    torch.cuda.synchronize()
    assert C.untouched()


# ------------------------------------------------------------------------------------------------------------- LayerNorm
def _layernorm_launch(x, D, bar):
    """In-place LayerNorm of x [M, D] inside a canvas whose slack (the rows in front of it and after row M) holds the sentinel."""
    from rohm_amd import ops
    g, b = seeded(1, D), seeded(2, D)
    ref = nets.layer_norm(x.double(), g.double(), b.double())
    X = Canvas(x.shape[0], D, fill=SENTINEL, data=x)
    (G, g_v), (B, b_v) = _vec(g), _vec(b)
    ops.layernorm_(X.view, g_v, b_v)
    err, finite = _window_error(X.view, ref)
    assert X.outside_untouched(), 'rows that are not this launch\'s were written'
    assert G.untouched() and B.untouched()
    assert finite and err < bar, (err, bar)
    return err, X.view.cpu(), b


@pytest.mark.parametrize('D', [256, 512, 1024])
@pytest.mark.parametrize('M', [1, 3, 4, 5, 1000])      # a workgroup is 4 rows: 1, 3 and 5 leave waves of the last one idle
def test_layernorm_widths_and_row_tails(M, D):
    err, _, _ = _layernorm_launch(seeded(M, M, D) * 3 + 0.5, D, 5e-6)
    _note('layernorm (e)', err)


@pytest.mark.parametrize('D', [256, 512, 1024])
def test_layernorm_constant_rows(D):
    """Rows of one value: sums of equal values are exact at every level of the reduction (multiples of the value below 2^24), so the
    mean is the value, every deviation 0 and the result beta -- not 0 / 0."""
    x = seeded(D, 7, D) * 3 + 0.5
    x[1], x[3], x[4] = 0.0, 1.0, 600.0
    err, out, beta = _layernorm_launch(x, D, 5e-6)
    for r in (1, 3, 4):
        assert bool(torch.isfinite(out[r]).all()) and float((out[r] - beta).abs().max()) < 1e-6
    _note('layernorm (e)', err)


@pytest.mark.parametrize('D', [256, 512, 1024])
def test_layernorm_rows_far_from_zero(D):
    """Mean 600, unit variance: the bar of test_gemm_res_layernorm_rows_far_from_zero (fp32 resolution of x ~ 600 is 6e-5)."""
    err, _, _ = _layernorm_launch(seeded(D + 1, 5, D) + 600.0, D, 5e-4)
    _note('layernorm (e) rows at 600', err)


def test_layernorm_refuses_other_widths():
    from rohm_amd import _lib, ops
    X = Canvas(4, 768, fill=SENTINEL, data=seeded(0, 4, 768))
    with pytest.raises(_lib.RohmHipError, match='768'):
        ops.layernorm_(X.view, torch.ones(768, device=_dev()), torch.zeros(768, device=_dev()))
    torch.cuda.synchronize()
    assert X.untouched()


# ------------------------------------------------------------------------------------------------------------- attention
def _attention_launch(qkv, n_seq, n_head, S, dh):
    """qkv (q pre-scaled) in a NaN-padded canvas, ctx into a sentinel canvas -> error against float64 softmax(q k^T) v."""
    from rohm_amd import ops
    D = n_head * dh
    q, k, v = qkv.double().view(n_seq, S, 3, n_head, dh).permute(2, 0, 3, 1, 4)
    ref = (torch.softmax(q @ k.transpose(-1, -2), dim=-1) @ v).permute(0, 2, 1, 3).reshape(n_seq * S, D)
    Q = Canvas(n_seq * S, 3 * D, data=qkv)
    C = Canvas(n_seq * S, D, fill=SENTINEL)
    out = ops.attention(Q.view, n_seq, n_head, S, dh, out=C.view)
    assert out.data_ptr() == C.view.data_ptr()
    err, finite = _window_error(C.view, ref)
    assert C.outside_untouched(), 'the kernel wrote outside ctx'
    assert Q.untouched()
    assert finite and err < 5e-6, err
    return err


@pytest.mark.parametrize('dh', [64, 128])
@pytest.mark.parametrize('S', [1, 63, 65, 128, 129, 300])      # around the 64-key chunk and the 64-query group; 300: five chunks
def test_attention_general_around_its_chunk(S, dh):
    n_head = 2
    for n_seq in (1, 3):
        qkv = seeded(n_seq * 7 + S, n_seq * S, 3 * n_head * dh)
        qkv[:, :n_head * dh] *= dh ** -0.5
        _note('attention (f) general', _attention_launch(qkv, n_seq, n_head, S, dh))


@pytest.mark.parametrize('n_seq', [1, 33])      # split and full launch shapes
def test_attention_specialised_writes_ctx_only(n_seq):
    n_head = 4
    qkv = seeded(n_seq * 10 + n_head, n_seq * 144, 3 * n_head * 128)
    qkv[:, :n_head * 128] *= 128 ** -0.5
    _note('attention (f) specialised', _attention_launch(qkv, n_seq, n_head, 144, 128))
