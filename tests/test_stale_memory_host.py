"""Host side of the stale-memory tests (tests/test_gpu_stale_memory.py): the poisoning replacement of torch's uninitialised
allocators really poisons and really goes away, and every entry point of the public headers (rohm_amd._lib.HEADERS) that is
handed a caller-owned buffer is run by a case of that module."""
import numpy as np
import pytest
import torch

import stale_memory as SM


@pytest.mark.parametrize('name', sorted(SM.PATTERNS))
def test_poisoned_allocators_return_the_pattern_and_are_restored(name, monkeypatch):
    word = SM.PATTERNS[name]
    real = (torch.empty, torch.empty_like, torch.Tensor.new_empty)
    want32 = int(np.frombuffer(word, dtype='<u4')[0])
    with monkeypatch.context() as m:
        SM.install(m, word, device_types=('cpu',))
        assert torch.empty is not real[0] and torch.empty_like is not real[1] and torch.Tensor.new_empty is not real[2]
        a = torch.empty(5, 3, dtype=torch.float32)
        b = torch.empty_like(torch.zeros(7, dtype=torch.int32))
        c = torch.zeros(2, dtype=torch.float64).new_empty((3, 2))
        d = torch.empty(6, dtype=torch.uint8)                       # not a whole number of words
        e = torch.empty_like(torch.zeros(4, 6).t())                 # preserve_format: dense, not contiguous
        f = torch.empty((), dtype=torch.float32)
        g = torch.empty(0, 4)
        for t, n in ((a, 15), (b, 7), (c, 12), (e, 24), (f, 1)):
            words = np.frombuffer(SM.bits(t).numpy().tobytes(), dtype='<u4')
            assert words.shape == (n,) and (words == want32).all(), (name, t.dtype)
        assert SM.bits(d).tolist() == list((word * 2)[:6])
        assert g.numel() == 0 and c.dtype == torch.float64 and e.stride() == (1, 6)
        if name == 'ones':
            assert torch.isnan(a).all() and torch.isnan(c).all() and int(b[0]) == -1
        if name == 'fltmax':
            assert float(a[0, 0]) == float(np.finfo(np.float32).max)
        if name == 'small':
            assert 0.0 < float(a[0, 0]) < 1e-37 and int(b[0]) == 0x01010101
        z = torch.zeros(4)                                           # torch.zeros is left alone
        assert float(z.abs().sum()) == 0.0
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == real


def test_only_the_named_device_types_are_filled(monkeypatch):
    filled = []
    real = SM.fill_bytes
    monkeypatch.setattr(SM, 'fill_bytes', lambda t, word: (filled.append(t.device.type), real(t, word))[1])
    with SM.poison(SM.PATTERNS['small']):                           # default: device tensors only -- a CPU tensor is not touched
        torch.empty(4, dtype=torch.int32)
        torch.empty_like(torch.zeros(3))
        torch.zeros(2).new_empty((5,))
    assert filled == []
    with SM.poison(SM.PATTERNS['small'], device_types=('cpu',)):
        t = torch.empty(4, dtype=torch.int32)
    assert filled == ['cpu'] and t.tolist() == [0x01010101] * 4


def test_bit_comparison_sees_nan_payloads_and_signed_zeros():
    a = torch.tensor([float('nan'), 0.0, 1.0])
    assert SM.first_difference(a, a.clone()) is None
    b = a.clone()
    b[1] = -0.0
    assert SM.first_difference(a, b)[0] == 1
    c = a.clone()
    c.view(torch.int32)[0] ^= 1                                      # another NaN
    assert SM.first_difference(a, c)[0] == 0


def test_the_header_parser_finds_the_buffer_taking_entry_points():
    fns = SM.abi_buffer_functions()
    assert len(fns) >= 24 and sum(len(v) for v in fns.values()) >= 26, sorted(fns)      # (as of this test; the guard test below names what is new)
    assert set(n for names in fns.values() for n in names) >= {'scratch', 'ws', 'saved', 'buf'}
    assert fns['rohm_posenet_train_backward'] == ['saved', 'scratch'] and fns['rohm_posenet_set_stack_timeline'] == ['buf']
    sample = 'int rohm_x(const float* a, void* ws, size_t ws_bytes);\nint rohm_y(void* p, size_t n);\n/* int rohm_z(void* ws, size_t ws_bytes); */'
    assert SM.abi_buffer_functions(sample) == {'rohm_x': ['ws']}


def test_every_buffer_taking_entry_point_is_covered_by_a_case():
    """Completeness guard: a new entry point with a caller-owned buffer needs a case in tests/test_gpu_stale_memory.py."""
    import test_gpu_stale_memory as G
    from rohm_amd import _lib
    fns = set(SM.abi_buffer_functions())
    covered = SM.covered_functions()
    assert len(SM.EXEMPT) <= 2 and set(SM.EXEMPT) <= fns and not set(SM.EXEMPT) & covered
    missing = fns - covered - set(SM.EXEMPT)
    assert not missing, f'no stale-memory case runs {sorted(missing)}'
    assert covered <= set(_lib.SIGNATURES), sorted(covered - set(_lib.SIGNATURES))
    # the coverage list is about cases that exist: every family has at least one case, every case belongs to a family
    families = {G.family(name) for name in G.CASES}
    assert families == set(SM.COVERAGE), (sorted(families - set(SM.COVERAGE)), sorted(set(SM.COVERAGE) - families))
