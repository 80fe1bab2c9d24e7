"""Host side of the stream-order tests (tests/test_gpu_stream_order.py), on the CPU: the header parser for stream-taking entry
points, the lists that class each of them (run and proven by a case, documented as waiting, exempt), the sentences those lists
quote, the bookkeeping of deferred inputs on CPU tensors, the gate's arithmetic on a clock that the test moves, and the call
log's install and restore on a stand-in object."""
import contextlib
import ctypes as C

import pytest
import torch

import stale_memory as SM
import stream_order as SO


# ---- the header -------------------------------------------------------------------------------------------------------------------------
def test_the_header_parser_finds_the_stream_taking_entry_points():
    sample = ('int rohm_a(const float* x, int n, double* out, rohm_stream_t stream);\n'
              'int rohm_b(rohm_stream_t s, const float* x);\n'
              'int rohm_c(const rohm_posenet_t* h,\n           void* ws, size_t ws_bytes,\n           rohm_stream_t stream);\n'
              '/* int rohm_d(float* x, rohm_stream_t stream); */\nsize_t rohm_e(int M, int N);\n// int rohm_f(rohm_stream_t stream);\n'
              'typedef void* rohm_stream_t;\nint rohm_g(const rohm_stream_t stream);\n')
    assert SO.abi_stream_functions(sample) == {'rohm_a': 3, 'rohm_b': 0, 'rohm_c': 3, 'rohm_g': 0}
    with pytest.raises(ValueError):
        SO.abi_stream_functions('int rohm_two(rohm_stream_t a, rohm_stream_t b);')
    fns = SO.abi_stream_functions()
    assert len(fns) >= 78, sorted(fns)                                            # (as of this test; the guard test below names what is new)
    assert fns['rohm_ddpm_step'] == 10 and fns['rohm_posenet_forward'] == 9 and fns['rohm_trajnet_sample_loop'] == 14
    assert not {'rohm_posenet_create', 'rohm_trajnet_create', 'rohm_smplx_create', 'rohm_profile_stop', 'rohm_exchange_probe',
                'rohm_posenet_set_exchange', 'rohm_posenet_workspace_bytes'} & set(fns)


def test_the_stream_positions_agree_with_the_ctypes_signatures():
    from rohm_amd import _lib
    for name, at in SO.abi_stream_functions().items():
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and args[at] is C.c_void_p, name
        assert at == len(args) - 1, name                                          # (today every entry point takes its stream last)


def test_every_stream_taking_entry_point_is_classed_once():
    """Completeness guard: a new entry point with a stream parameter needs a case (tests/test_gpu_stale_memory.py::CASES or
    tests/test_gpu_bounds.py::EXTRA, which tests/test_gpu_stream_order.py runs behind a gate), a header sentence in SYNC_DOCUMENTED, or a
    reason in STREAM_EXEMPT.  The classes: documented as waiting; else exempt; else run by a case and held to wait-free there."""
    import test_gpu_bounds as B
    fns = set(SO.abi_stream_functions())
    run = SM.covered_functions() | {f for fs in B.EXTRA_COVERAGE.values() for f in fs}
    documented, exempt = set(SO.SYNC_DOCUMENTED) & fns, set(SO.STREAM_EXEMPT)
    assert exempt <= fns and not exempt & run and not exempt & set(SO.SYNC_DOCUMENTED)
    assert all(len(reason) > 20 for reason in SO.STREAM_EXEMPT.values())
    held = (run & fns) - documented
    classes = {f: [f in held, f in documented, f in exempt] for f in fns}
    assert all(sum(c) == 1 for c in classes.values()), {f: c for f, c in classes.items() if sum(c) != 1}
    # the functions documented as waiting are known by name; what the call log cannot see (no stream parameter) is listed for the record
    assert documented == {'rohm_posenet_exchange_status', 'rohm_trajnet_sample_loop', 'rohm_track_resample', 'rohm_floor_hypotheses'}
    assert set(SO.SYNC_DOCUMENTED) - fns == {'rohm_posenet_create', 'rohm_trajnet_create', 'rohm_smplx_create', 'rohm_exchange_probe',
                                             'rohm_posenet_set_exchange', 'rohm_profile_stop'}
    assert set(SO.SYNC_ONLY_IN) <= documented
    # a function that waits in one form only is still run in the other: the registry has wait-free cases of it
    import test_gpu_stale_memory as G
    for f, applies in SO.SYNC_ONLY_IN.items():
        fams = [fam for fam, fs in SM.COVERAGE.items() if f in fs]
        names = [n for n in G.CASES if G.family(n) in fams]
        assert any(applies(n) for n in names) and any(not applies(n) for n in names), f
        assert SO.may_wait(f, next(n for n in names if applies(n))) and not SO.may_wait(f, next(n for n in names if not applies(n)))
    assert SO.may_wait('rohm_track_resample', 'any case') and not SO.may_wait('rohm_ddpm_step', 'any case')


def test_every_documented_wait_quotes_a_sentence_of_the_header():
    prose = SO.header_prose()
    for f, sentence in SO.SYNC_DOCUMENTED.items():
        assert len(sentence) > 40 and sentence in prose, f
        assert f in sentence or '*_create' in sentence or f in prose[max(0, prose.index(sentence) - 1500):prose.index(sentence) + 3000], f
    assert SO.header_prose('/* a\n * b\n   * c */\nint x;') == '/* a b c */ int x;'
    assert 'tests/test_gpu_stream_order.py holds every entry point to this' in prose


# ---- deferred inputs --------------------------------------------------------------------------------------------------------------------
def test_prefill_is_nan_for_floats_and_a_valid_index_for_integers():
    for dtype in (torch.float32, torch.float64, torch.float16):
        assert SO.prefill_word(dtype) == b'\xff\xff\xff\xff'
    for dtype in (torch.int32, torch.int64, torch.uint8, torch.bool, torch.int16):
        assert SO.prefill_word(dtype) == b'\x00\x00\x00\x00'


def test_deferred_inputs_are_prefilled_staged_and_copied_in_sequence():
    a = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    i = torch.tensor([3, 1, 2], dtype=torch.int64)
    m = torch.tensor([True, False, True])
    d = torch.arange(5, dtype=torch.float64)
    inputs = SO.DeferredInputs('cpu')
    for t in (a, i, m, d):
        got = inputs.record(t)
        assert got.data_ptr() == t.data_ptr()                                     # `_d` of a plain run: the tensor on the device
    a_before = a.clone()
    inputs.stage()
    assert len(inputs.staged) == 4 and not inputs.complete()
    dst = [dst for _, dst in inputs.staged]
    assert torch.isnan(dst[0]).all() and torch.isnan(dst[3]).all() and dst[1].tolist() == [0, 0, 0] and dst[2].tolist() == [False] * 3
    assert [tuple(x.shape) for x in dst] == [(3, 4), (3,), (3,), (5,)] and [x.dtype for x in dst] == [t.dtype for t in (a, i, m, d)]
    assert all(src.data_ptr() != t.data_ptr() for (src, _), t in zip(inputs.staged, (a, i, m, d)))       # staged copies, not the inputs
    armed = []
    out = inputs.replay(a.clone(), before_copy=lambda: armed.append(inputs.replayed))
    assert out.data_ptr() == dst[0].data_ptr() and torch.equal(out, a_before) and armed == [0]
    assert torch.isnan(dst[3]).all()                                              # nothing is copied before it is asked for
    with pytest.raises(AssertionError, match='input #1'):                         # another shape
        inputs.replay(torch.tensor([3, 1], dtype=torch.int64))
    with pytest.raises(AssertionError, match='input #1'):                         # another dtype
        inputs.replay(i.to(torch.int32))
    with pytest.raises(AssertionError, match='input #1 differs'):                 # another value
        inputs.replay(torch.tensor([3, 1, 5], dtype=torch.int64))
    assert inputs.replayed == 1 and dst[1].tolist() == [0, 0, 0]
    assert inputs.replay(i.clone()).tolist() == [3, 1, 2] and inputs.replay(m.clone()).tolist() == [True, False, True]
    assert torch.equal(inputs.replay(d.clone()), d) and inputs.complete()
    with pytest.raises(AssertionError, match='asks for input #4'):                # one more than the plain run
        inputs.replay(d.clone())
    with pytest.raises(AssertionError, match='not contiguous'):
        SO.DeferredInputs('cpu').record(torch.zeros(4, 6).t())


def test_a_nan_input_compares_equal_to_itself_in_the_sequence_check():
    x = torch.tensor([float('nan'), 1.0])
    inputs = SO.DeferredInputs('cpu')
    inputs.record(x)
    inputs.stage()
    assert SM.first_difference(inputs.replay(x.clone()), x) is None


# ---- the gate and the call log ----------------------------------------------------------------------------------------------------------
class _Clock:
    def __init__(self):
        self.t = 100.0

    def __call__(self):
        return self.t


class _Device:
    """A stand-in device: delays queue up one behind the other from the moment they are armed; an event completes with the delay it
    was recorded behind."""

    def __init__(self, clock):
        self.clock, self.busy_until, self.delays = clock, 0.0, []

    def delay(self, units):
        self.delays.append(units)
        self.busy_until = max(self.busy_until, self.clock()) + units / 1000.0         # 1 unit per millisecond below

    def event(self):
        dev = self

        class Event:
            def record(self, stream):
                self.done_at = dev.busy_until

            def query(self):
                return dev.clock() >= self.done_at
        return Event()

    def synchronize(self):
        self.clock.t = max(self.clock.t, self.busy_until)


def _gates(length=0.020):
    clock = _Clock()
    dev = _Device(clock)
    return SO.Gates('side', length, dev.delay, 1.0, event=dev.event, clock=clock, on_stream=lambda s: contextlib.nullcontext()), dev, clock


def test_a_further_gate_is_armed_when_the_host_clock_says_less_than_asked_for_may_be_left():
    gates, dev, clock = _gates()
    assert not gates.closed() and gates.may_remain() < 0
    gates.ensure_gate(0.010)
    assert gates.count == 1 and gates.closed() and dev.delays == [20.0] and abs(gates.may_remain() - 0.020) < 1e-9
    clock.t += 0.009
    gates.ensure_gate(0.010)                                                      # 11 ms left: enough
    assert gates.count == 1
    clock.t += 0.002
    gates.ensure_gate(0.010)                                                      # 9 ms left: a further gate, queued behind the first
    assert gates.count == 2 and gates.closed() and abs(dev.busy_until - (100.0 + 0.040)) < 1e-9
    assert abs(gates.may_remain() - 0.020) < 1e-9                                 # (a lower bound: the device will hold it for 29 ms)
    dev.synchronize()                                                             # a wait drains every gate
    assert not gates.closed() and gates.may_remain() < 0
    gates.ensure_gate(0.010)
    assert gates.count == 3 and gates.closed()
    with pytest.raises(ValueError):
        gates.ensure_gate(0.020)                                                  # a gate can never have its whole length left


def test_the_call_log_installs_records_and_restores():
    gates, dev, clock = _gates()
    current = [0x1234]

    class Lib:
        def __init__(self):
            self.seen = []

        def rohm_launch(self, x, stream):
            clock.t += 0.001                                                      # a millisecond of enqueue
            self.seen.append(('launch', x))
            return 0

        def rohm_wait(self, stream, x):
            dev.synchronize()
            return -7

        def rohm_other(self, x):
            return 5

    lib = Lib()
    log = SO.CallLog(gates, 0.010, current_stream=lambda: current[0], clock=clock)
    with log.installed(lib, {'rohm_launch': 1, 'rohm_wait': 0}):
        assert lib.rohm_launch.__wrapped__.__func__ is Lib.rohm_launch and 'rohm_other' not in vars(lib)
        assert lib.rohm_launch('a', C.c_void_p(0x1234)) == 0 and gates.count == 1
        assert lib.rohm_wait(0x1234, 'b') == -7                                   # the return value passes through
        assert lib.rohm_launch('c', 0x1234) == 0 and gates.count == 2             # the drained gate was replaced before the call
        with pytest.raises(AssertionError, match=r'rohm_launch was handed the stream 0x0, the current stream is 0x1234'):
            lib.rohm_launch('d', None)
        with pytest.raises(AssertionError, match='rohm_wait was handed the stream 0x99'):
            lib.rohm_wait(C.c_void_p(0x99), 'e')
        current[0] = 0                                                            # the null stream: None, 0 and c_void_p(None) all name it
        assert lib.rohm_launch('f', None) == 0 and lib.rohm_launch('g', C.c_void_p(None)) == 0
    assert lib.rohm_launch.__func__ is Lib.rohm_launch and lib.rohm_wait.__func__ is Lib.rohm_wait
    assert lib.seen == [('launch', 'a'), ('launch', 'c'), ('launch', 'f'), ('launch', 'g')]     # a refused call never reached the library
    assert [(f, closed) for f, _, closed in log.calls] == [('rohm_launch', True), ('rohm_wait', False), ('rohm_launch', True),
                                                           ('rohm_launch', True), ('rohm_launch', True)]
    assert abs(log.calls[0][1] - 0.001) < 1e-9 and log.calls[1][1] >= 0.018       # host seconds: the wait took what was left of the gate
    assert log.functions() == {'rohm_launch', 'rohm_wait'} and log.proven() == {'rohm_launch'}
    assert [f for f, _ in log.unproven()] == ['rohm_wait'] and log.unproven(lambda f: f == 'rohm_wait') == []
    assert log.slowest()[1] == 'rohm_wait' and log.slowest(skip={'rohm_wait'})[1] == 'rohm_launch' and abs(log.slowest(skip={'rohm_wait'})[0] - 0.001) < 1e-9
    assert SO.CallLog().slowest() == (0.0, None)


def test_the_originals_come_back_after_an_exception_and_a_plain_log_notes_no_gate():
    class Lib:
        def rohm_x(self, stream):
            return 1
    lib, log = Lib(), SO.CallLog(current_stream=lambda: 0)
    with pytest.raises(RuntimeError):
        with log.installed(lib, {'rohm_x': 0}):
            assert lib.rohm_x(None) == 1
            raise RuntimeError('the case failed')
    assert lib.rohm_x.__func__ is Lib.rohm_x
    assert [(f, closed) for f, _, closed in log.calls] == [('rohm_x', None)] and log.unproven() == [] and log.proven() == set()
    with pytest.raises(AttributeError):                                           # a name the library does not have is an error, and
        with log.installed(lib, {'rohm_x': 0, 'rohm_missing': 0}):                # what was installed before it is put back
            pass
    assert lib.rohm_x.__func__ is Lib.rohm_x


def test_stream_values():
    assert SO.stream_value(None) == 0 and SO.stream_value(0) == 0 and SO.stream_value(C.c_void_p(None)) == 0
    assert SO.stream_value(C.c_void_p(0x7f00)) == 0x7f00 and SO.stream_value(0x7f00) == 0x7f00
