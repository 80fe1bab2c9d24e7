"""Host side of the guarded-memory tests (tests/test_gpu_bounds.py), on CPU tensors: the guarded allocators return what was asked for
inside intact bands and go away again, a store one element outside a view is reported with its offset, a load there is NaN, inputs
placed on a canvas round-trip and a change of one bit is noticed; and every entry point of the public headers that can be handed a
caller's tensor is run by a guarded-memory case or exempt by name."""
import pytest
import torch

import guarded_memory as GM
import stale_memory as SM

CPU = ('cpu',)
DTYPES = (torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8)


def _outside(t, element):
    """A one-element view `element` elements away from the first element of the contiguous tensor `t` (-1: just in front of it,
    t.numel(): just behind it), through torch.as_strided."""
    return torch.as_strided(t, (1,), (1,), t.storage_offset() + element)


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: str(d).replace('torch.', ''))
def test_every_form_returns_the_shape_dtype_zeros_and_alignment_asked_for(dtype):
    real = (torch.empty, torch.empty_like, torch.Tensor.new_empty, torch.zeros, torch.Tensor.new_zeros, SM.fill_bytes)
    proto = torch.ones(3, dtype=dtype)
    with GM.guard(CPU) as g:
        made = [('empty ints', torch.empty(5, 3, dtype=dtype), (5, 3)), ('empty tuple', torch.empty((7,), dtype=dtype), (7,)),
                ('empty size=', torch.empty(size=(2, 3, 4), dtype=dtype), (2, 3, 4)), ('empty scalar', torch.empty((), dtype=dtype), ()),
                ('empty 0', torch.empty(0, 4, dtype=dtype), (0, 4)), ('zeros', torch.zeros(4, 6, dtype=dtype), (4, 6)),
                ('zeros list', torch.zeros([9], dtype=dtype), (9,)), ('empty_like', torch.empty_like(torch.ones(6, 2, dtype=dtype)), (6, 2)),
                ('empty_like contiguous', torch.empty_like(torch.ones(4, 6, dtype=dtype).t(), memory_format=torch.contiguous_format), (6, 4)),
                ('new_empty', proto.new_empty((3, 2)), (3, 2)), ('new_empty ints', proto.new_empty(2, 5), (2, 5)),
                ('new_zeros', proto.new_zeros((11,)), (11,)), ('new_empty dtype', torch.ones(2).new_empty((4,), dtype=dtype), (4,))]
        for what, t, shape in made:
            assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous(), what
            assert t.data_ptr() % GM.ALIGN == 0 or t.numel() == 0, what
            assert not t.any(), what                                             # the interior is zero-filled
        kept = torch.empty_like(torch.ones(4, 6, dtype=dtype).t())               # preserve_format: dense, not contiguous
        assert kept.stride() == (1, 6) and tuple(kept.shape) == (6, 4) and kept.data_ptr() % GM.ALIGN == 0 and not kept.any()
        assert g.served == len(made) + 1 and g.unguarded == 0 and len(g.log()) == g.served
        assert g.log()[0] == ('empty', (5, 3), dtype, 15 * proto.element_size())
        assert g.violations() == []
        for _, t, _ in made:                                                      # writing all of the interior is no violation
            t.fill_(1)
        assert g.violations() == []
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty, torch.zeros, torch.Tensor.new_zeros, SM.fill_bytes) == real


def test_the_default_device_types_leave_cpu_tensors_alone():
    with GM.guard() as g:
        torch.empty(4)
        torch.zeros(3).new_zeros((2,))
    assert g.served == 0 and g.unguarded == 0


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: str(d).replace('torch.', ''))
def test_a_store_one_element_outside_is_reported_with_its_offset_and_a_load_there_is_nan(dtype):
    size = torch.empty((), dtype=dtype).element_size()
    with GM.guard(CPU) as g:
        a, b, c = torch.empty(5, 3, dtype=dtype), torch.zeros(130, dtype=dtype), torch.empty(8, dtype=dtype)
        before, behind = _outside(a, -1), _outside(a, a.numel())
        if dtype.is_floating_point:
            assert torch.isnan(before).all() and torch.isnan(behind).all()      # a load from a band is NaN ...
        else:
            assert int(before) == (255 if dtype == torch.uint8 else -1)          # ... or the all-ones integer
        assert g.violations() == []
        behind.fill_(3)                                                           # one element past the end of `a`
        _outside(b, -1).fill_(0)                                                  # one element in front of `b`
        got = g.violations()
        assert [(i, off) for i, _, off in got] == [(0, 15 * size), (1, -size)], got
        assert 'empty[5, 3]' in got[0][1] and 'zeros[130]' in got[1][1]
        r = g.records[2]
        _outside(c, (r.flat.numel() - r.front) // size - 1).fill_(0)              # the very last band element is still watched
        assert [i for i, _, _ in g.violations()] == [0, 1, 2]


def test_the_pad_bytes_behind_an_interior_that_is_no_multiple_of_512_are_band():
    with GM.guard(CPU) as g:
        t = torch.empty(3, dtype=torch.uint8)
        _outside(t, 3).fill_(0)
        assert [(i, off) for i, _, off in g.violations()] == [(0, 3)]
        r = g.records[0]
        assert r.front >= GM.BAND and r.flat.numel() - r.front - r.nbytes >= GM.BAND + GM.ALIGN - 3


def test_allocations_that_cannot_be_served_are_passed_through_and_counted():
    with GM.guard(CPU) as g:
        out = torch.ones(6)
        a = torch.empty(6, out=out)
        b = torch.empty(2, 3, 4, 5, memory_format=torch.channels_last)
        c = torch.empty_like(torch.ones(2, 3, 4, 5), memory_format=torch.channels_last)
        d = torch.empty_like(torch.ones(4, 4)[:, ::2])                           # preserve_format of a tensor with holes
        e = torch.zeros(3)                                                        # served
        assert a.data_ptr() == out.data_ptr() and b.is_contiguous(memory_format=torch.channels_last) and tuple(c.shape) == (2, 3, 4, 5)
        assert tuple(d.shape) == (4, 2) and not e.any()
        assert g.unguarded == 4 and g.served == 1, g.passed_through
        assert ['out=' in g.passed_through[0], 'channels_last' in g.passed_through[1], 'channels_last' in g.passed_through[2],
                'not dense' in g.passed_through[3]] == [True] * 4, g.passed_through


def test_poisoning_inside_a_guard_fills_the_interior_and_leaves_the_bands():
    """A case may poison its own set-up (`with SM.poison(SM.ZEROS)` in clips_repr): stale_memory.fill_bytes fills the whole storage,
    which under a guard would wipe the bands."""
    with GM.guard(CPU) as g:
        with SM.poison(SM.PATTERNS['small'], device_types=CPU):
            t = torch.empty(5, dtype=torch.int32)
        assert t.tolist() == [0x01010101] * 5 and t.data_ptr() % GM.ALIGN == 0
        assert g.served == 1 and g.violations() == []
    with SM.poison(SM.PATTERNS['small'], device_types=CPU):                      # and outside a guard it is what it was
        assert torch.empty(3, dtype=torch.int32).tolist() == [0x01010101] * 3


@pytest.mark.parametrize('dtype', DTYPES + (torch.bool, torch.int16), ids=lambda d: str(d).replace('torch.', ''))
def test_place_round_trips_and_untouched_notices_one_bit(dtype):
    src = (torch.arange(35).reshape(5, 7) % 2).to(dtype) if dtype == torch.bool else torch.arange(35).reshape(5, 7).to(dtype)
    canv = []
    t = GM.place(src, 'aligned', into=canv, label='src')
    c = canv[0]
    assert t.dtype == dtype and tuple(t.shape) == (5, 7) and torch.equal(t, src) and t.data_ptr() % GM.ALIGN == 0
    assert c.untouched() and c.bands_untouched() and c.first_change() is None and 'src[5, 7]' in c.describe()
    assert c.offset >= GM.BAND and c.flat.numel() - c.offset - c.nbytes >= GM.BAND
    if dtype.is_floating_point:
        assert torch.isnan(_outside(t, -1)).all() and torch.isnan(_outside(t, t.numel())).all()
    raw = t.view(torch.uint8) if dtype != torch.bool else c.flat[c.offset:c.offset + c.nbytes]
    raw.reshape(-1)[9] ^= 1                                                       # one bit of the operand
    assert not c.untouched() and c.bands_untouched() and c.first_change() == 9
    raw.reshape(-1)[9] ^= 1
    assert c.untouched()
    c.flat[c.offset + c.nbytes] ^= 0x10                                           # one bit just behind it
    assert not c.untouched() and not c.bands_untouched() and c.first_change() == c.nbytes


def test_slice_placement_is_a_batch_slice_eight_bytes_past_a_sixteen_byte_boundary():
    for T in (143, 63):
        src = torch.arange(2 * 294 * T, dtype=torch.float32).reshape(2, 294, 1, T)
        canv = []
        t = GM.place(src, 'slice', into=canv)
        c = canv[0]
        assert torch.equal(t, src) and t.is_contiguous() and t.data_ptr() % 16 == 8
        assert (t.data_ptr() - 294 * T * 4) % GM.ALIGN == 0                       # the canvas's clip 0 is aligned ...
        assert torch.isnan(torch.as_strided(t, (294 * T,), (1,), t.storage_offset() - 294 * T)).all()      # ... and all NaN
        assert c.untouched() and torch.isnan(_outside(t, t.numel())).all()
    with pytest.raises(ValueError):
        GM.place(torch.zeros(2, 13, 16), 'slice')
    with pytest.raises(ValueError):
        GM.place(torch.zeros(4, 6).t(), 'aligned')


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: str(d).replace('torch.', ''))
def test_offset_placement_and_the_offset_guard_start_one_element_past_a_boundary(dtype):
    size = torch.empty((), dtype=dtype).element_size()
    src, canv = torch.arange(35).reshape(5, 7).to(dtype), []
    t = GM.place(src, 'offset', into=canv, label='src')
    c = canv[0]
    assert torch.equal(t, src) and t.is_contiguous() and t.data_ptr() % GM.ALIGN == size and '(offset)' in c.describe()
    assert c.untouched() and c.offset >= GM.BAND + size and c.flat.numel() - c.offset - c.nbytes >= GM.BAND
    _outside(t, -1).fill_(0)                                                      # the element between the boundary and the operand is band
    assert not c.bands_untouched() and c.first_change() == -size
    with GM.guard(CPU, offset=True) as g:
        a, z = torch.empty(5, 3, dtype=dtype), torch.ones(2, dtype=dtype).new_zeros((4,))
        assert a.data_ptr() % GM.ALIGN == size and z.data_ptr() % GM.ALIGN == size and not a.any() and not z.any()
        a.fill_(1)
        assert g.violations() == [] and g.served == 2 and g.unguarded == 0
        _outside(a, -1).fill_(0)
        _outside(z, 4).fill_(0)
        assert [(i, off) for i, _, off in g.violations()] == [(0, -size), (1, 4 * size)]
    with GM.guard(CPU) as g:                                                      # and without the option allocations are aligned as before
        assert torch.empty(3, dtype=dtype).data_ptr() % GM.ALIGN == 0


def test_another_band_word_is_kept_around_the_operand():
    canv = []
    t = GM.place(torch.ones(6), 'aligned', into=canv, band=b'\x01\x00\xc0\x7f')
    assert torch.isnan(_outside(t, -1)).all() and _outside(t, 6).view(torch.int32).item() == 0x7FC00001 and canv[0].untouched()


# ---- the header -------------------------------------------------------------------------------------------------------------------------
def test_the_header_parser_finds_the_pointer_taking_entry_points():
    sample = ('int rohm_a(const float* x, int n, double* out, rohm_stream_t s);\n'
              'int rohm_b(const rohm_posenet_t* h, const char** why);\n'
              'int rohm_c(float* const* params, const float* const* grads, const long long* numel, unsigned char* gap, const int32_t* idx,\n'
              '           const unsigned* bits, void* ws, size_t ws_bytes);\n'
              '/* int rohm_d(float* x); */\nsize_t rohm_e(int M, int N);\nvoid rohm_f(rohm_smplx_t* h);\n')
    assert SM.abi_pointer_functions(sample) == {'rohm_a': ['x', 'out'], 'rohm_c': ['params', 'grads', 'numel', 'gap', 'idx', 'bits', 'ws']}
    fns = SM.abi_pointer_functions()
    assert len(fns) >= 84, sorted(fns)                                            # (as of this test; the guard test below names what is new)
    assert set(SM.abi_buffer_functions()) <= set(fns)
    assert fns['rohm_ddpm_step'] == ['x_t', 'x0', 'noise', 'guid_grad', 'x_prev']
    assert fns['rohm_floor_moments'] == ['points', 'plane', 'origin', 'out']
    assert 'rohm_posenet_create' not in fns and 'rohm_trajnet_tune' not in fns and 'rohm_exchange_probe' not in fns


def test_every_pointer_taking_entry_point_is_run_by_a_guarded_case_or_exempt_by_name():
    """Completeness guard: a new entry point that can be handed a caller's tensor needs a case in tests/test_gpu_stale_memory.py (which
    tests/test_gpu_bounds.py runs under guards) or in tests/test_gpu_bounds.py::EXTRA_COVERAGE, or a reason in POINTER_EXEMPT."""
    import test_gpu_bounds as B
    from rohm_amd import _lib
    fns = set(SM.abi_pointer_functions())
    extra = {f for fs in B.EXTRA_COVERAGE.values() for f in fs}
    covered = SM.covered_functions() | extra
    assert set(SM.POINTER_EXEMPT) <= fns and not set(SM.POINTER_EXEMPT) & covered
    assert all(len(reason) > 20 for reason in SM.POINTER_EXEMPT.values())
    missing = fns - covered - set(SM.POINTER_EXEMPT)
    assert not missing, f'no guarded-memory case runs {sorted(missing)}'
    assert extra <= set(_lib.SIGNATURES) and extra <= fns, sorted(extra - fns)
    # the extra list is about cases that exist, and the module runs every case of the registry as well
    assert {B.G.family(name) for name in B.EXTRA} == set(B.EXTRA_COVERAGE)
    assert set(B.ALL) == set(B.G.CASES) | set(B.EXTRA) and not set(B.G.CASES) & set(B.EXTRA)
