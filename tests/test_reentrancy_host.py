"""Host side of the re-entrancy tests (tests/test_gpu_reentrancy.py), on the CPU: the operand table read from the headers, the ledger
over a stand-in library (overlapping and touching ranges, a synchronisation in between, the same stream, NULL optional outputs, a
function with two buffers, a deferred call, two threads), the ordering rule on hand-made entries, the interval arithmetic on stand-in
events, the two worker threads, and the sentences the exemption tables quote."""
import ctypes as C
import threading
import time

import pytest
import torch

import reentrancy as RE
import stale_memory as SM
import stream_order as SO

SAMPLE = ('typedef struct rohm_net rohm_net_t;\ntypedef void* rohm_stream_t;\n'
          'int rohm_fwd(const rohm_net_t* h, const float* x, float* y, float* opt, void* ws, size_t ws_bytes, rohm_stream_t stream);\n'
          'int rohm_two(const float* x, void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes, rohm_stream_t stream);\n'
          'int rohm_status(const rohm_net_t* h, void* ws, size_t ws_bytes, rohm_stream_t stream);\n'
          'int rohm_table(const float* const* grads, const int64_t* numel, float* out, rohm_stream_t stream);\n'
          'size_t rohm_ws_bytes(const rohm_net_t* h, int B);\n')


# ---- the header ------------------------------------------------------------------------------------------------------------------
def test_the_operand_table_classes_every_pointer_by_the_headers_const():
    ops = RE.abi_operands(SAMPLE)
    assert set(ops) == {'rohm_fwd', 'rohm_two', 'rohm_status', 'rohm_table'}                      # (no stream: not listed)
    assert ops['rohm_fwd'] == dict(stream=6, handle=0, operands=[('x', 1, None, False), ('y', 2, None, True), ('opt', 3, None, True),
                                                                 ('ws', 4, 5, True)])
    assert ops['rohm_two'] == dict(stream=5, handle=None, operands=[('x', 0, None, False), ('saved', 1, 2, True), ('scratch', 3, 4, True)])
    assert ops['rohm_table']['operands'] == [('numel', 1, None, False), ('out', 2, None, True)]     # the table of pointers is a host array


def test_the_operand_table_agrees_with_the_other_parsers_of_the_headers():
    ops, stream_at, sized, pointers = RE.abi_operands(), SO.abi_stream_functions(), SM.abi_buffer_functions(), SM.abi_pointer_functions()
    assert set(ops) == set(stream_at) and len(ops) >= 78
    tables = {}
    for name, op in ops.items():
        assert op['stream'] == stream_at[name]
        names = [n for n, _, _, _ in op['operands']]
        assert set(names) <= set(pointers.get(name, [])), name
        missing = set(pointers.get(name, [])) - set(names)
        if missing:
            tables[name] = sorted(missing)
        assert {n for n, _, b, _ in op['operands'] if b is not None} == set(sized.get(name, [])), name
        for _, at, bytes_at, _ in op['operands']:
            assert bytes_at is None or bytes_at == at + 1
    # what the ledger does not see: device memory reached through a host table of pointers (the flat optimiser and the training gradients)
    assert tables == {'rohm_adamw_step': ['exp_avg', 'exp_avg_sq', 'grads', 'params'], 'rohm_grad_norm': ['grads'],
                      'rohm_trajnet_train_backward': ['grads']}
    assert ops['rohm_posenet_forward']['handle'] == 0 and ops['rohm_ddpm_step']['handle'] is None
    assert ('ws', 8, 9, True) in ops['rohm_guidance_skating_grad']['operands'] and ('ws', 10, 11, True) in ops['rohm_smplx_forward']['operands']
    # the buffers a backward reads are read: `saved` is const there and written by the forward
    assert ('saved', 14, 15, False) in ops['rohm_posenet_train_backward']['operands']


def test_addresses_and_extents():
    x = C.c_int(5)
    assert RE.address(None) == 0 and RE.address(0x70) == 0x70 and RE.address(C.c_void_p(None)) == 0 and RE.address(C.c_void_p(0x7f00)) == 0x7f00
    assert RE.address(C.byref(x)) == C.addressof(x) and RE.address(C.pointer(x)) == C.addressof(x) and RE.address('text') == 0
    t = torch.zeros(6, 8)
    assert RE.extent_bytes(t) == 192 and RE.extent_bytes(t[:, :3]) == (5 * 8 + 2 + 1) * 4 and RE.extent_bytes(t[0:0]) == 0
    assert RE.extent_bytes(torch.zeros(3, dtype=torch.float64)) == 24


# ---- the ledger over a stand-in library --------------------------------------------------------------------------------------------
class _Lib:
    def __init__(self):
        self.seen = []

    def rohm_fwd(self, h, x, y, opt, ws, ws_bytes, stream):
        self.seen.append('fwd')
        return 0

    def rohm_two(self, x, saved, saved_bytes, scratch, scratch_bytes, stream):
        self.seen.append('two')
        return 0

    def rohm_status(self, h, ws, ws_bytes, stream):
        self.seen.append('status')
        return -9

    def rohm_table(self, grads, numel, out, stream):
        return 0

    def rohm_ws_bytes(self, h, B):
        return 64


def _ledger(**kw):
    current = [0x10]
    led = RE.Ledger(RE.abi_operands(SAMPLE), current_stream=lambda: current[0], **kw)
    return led, current, _Lib()


def _fwd(lib, current, stream, x, y, ws, ws_bytes=64, opt=None, h=0xAA):
    current[0] = stream
    return lib.rohm_fwd(C.c_void_p(h), x, y, opt, C.c_void_p(ws), ws_bytes, C.c_void_p(stream))


def test_the_ledger_records_thread_stream_handle_and_ranges_and_restores():
    led, current, lib = _ledger()
    with led.installed(lib, patch_torch=False):
        led.sizes.update({0x1000: 40, 0x2000: 40})
        assert _fwd(lib, current, 0x10, C.c_void_p(0x1000), C.c_void_p(0x2000), 0x9000) == 0
        assert lib.rohm_ws_bytes(None, 1) == 64 and 'rohm_ws_bytes' not in vars(lib)               # not a stream-taking function
        with pytest.raises(AssertionError, match=r'rohm_fwd was handed the stream 0x99, the current stream is 0x10'):
            lib.rohm_fwd(None, None, None, None, None, 0, C.c_void_p(0x99))
    assert lib.rohm_fwd.__func__ is _Lib.rohm_fwd and lib.seen == ['fwd']
    (e,) = led.calls()
    assert e['function'] == 'rohm_fwd' and e['thread'] == threading.get_ident() and e['stream'] == 0x10 and e['handle'] == 0xAA
    assert e['writes'] == [('y', 0x2000, 0x2028), ('ws', 0x9000, 0x9040)] and e['reads'] == [('x', 0x1000, 0x1028)]      # NULL `opt`: no range
    assert e['enter'] < e['leave'] and e['rc'] == 0 and not e['waits'] and not e['deferred']
    assert led.streams_of() == {'rohm_fwd': {0x10}}


def test_overlapping_ranges_on_two_streams_are_reported_and_touching_ones_are_not():
    led, current, lib = _ledger()
    with led.installed(lib, patch_torch=False):
        led.sizes.update({0x1000: 40, 0x2000: 40, 0x3000: 40})
        _fwd(lib, current, 0x10, C.c_void_p(0x1000), C.c_void_p(0x2000), 0x9000)
        _fwd(lib, current, 0x20, C.c_void_p(0x1000), C.c_void_p(0x3000), 0x9040)       # reads the same x; its ws STARTS where the other ends
        assert RE.conflicts(led.entries) == []
        _fwd(lib, current, 0x20, C.c_void_p(0x1000), C.c_void_p(0x3000), 0x903f)       # one byte earlier: the two workspaces share a byte
    found = RE.conflicts(led.entries)
    assert [(a['stream'], b['stream'], wn, on, lo, hi) for a, b, wn, on, lo, hi in found] == [(0x10, 0x20, 'ws', 'ws', 0x903f, 0x9040)]
    text = RE.report(led.entries)[0]
    assert 'rohm_fwd on stream 0x10' in text and 'writes `ws`' in text and '[0x903f, 0x9040), 1 bytes' in text and 'no host-visible' in text


def test_an_output_that_another_stream_reads_is_reported_in_either_order():
    for first, second in ((0x10, 0x20), (0x20, 0x10)):
        led, current, lib = _ledger()
        with led.installed(lib, patch_torch=False):
            led.sizes.update({0x1000: 40, 0x2000: 40, 0x3000: 40})
            calls = {0x10: lambda: _fwd(lib, current, 0x10, C.c_void_p(0x1000), C.c_void_p(0x2000), 0x9000),       # writes y = 0x2000
                     0x20: lambda: _fwd(lib, current, 0x20, C.c_void_p(0x2010), C.c_void_p(0x3000), 0xA000)}       # reads inside it
            led.sizes[0x2010] = 8
            calls[first]()
            calls[second]()
        (c,) = RE.conflicts(led.entries)
        assert (c[0]['stream'], c[1]['stream'], c[2], c[3], c[4], c[5]) == (0x10, 0x20, 'y', 'x', 0x2010, 0x2018)
        assert 'reads `x`' in RE.describe(c)


def test_the_same_stream_and_a_synchronisation_in_between_order_two_calls():
    led, current, lib = _ledger()
    with led.installed(lib, patch_torch=False):
        shared = lambda stream: _fwd(lib, current, stream, None, None, 0x9000)
        shared(0x10)
        shared(0x10)                                             # the same stream: stream order
        assert RE.conflicts(led.entries) == []
        led.note_sync(0x20, lambda: None)                        # a wait for ANOTHER stream orders nothing here
        shared(0x20)
        assert len(RE.conflicts(led.entries)) == 2               # both earlier calls against this one
    for covering in (None, 0x10):                                # the device, or the first call's stream
        led, current, lib = _ledger()
        with led.installed(lib, patch_torch=False):
            _fwd(lib, current, 0x10, None, None, 0x9000)
            led.note_sync(covering, lambda: None)
            _fwd(lib, current, 0x20, None, None, 0x9000)
            assert RE.conflicts(led.entries) == []
            _fwd(lib, current, 0x10, None, None, 0x9000)         # ... but nothing orders the second stream's call before this one
            assert len(RE.conflicts(led.entries)) == 1


def test_a_documented_wait_orders_what_was_queued_before_it_and_not_itself():
    led, current, lib = _ledger(waits=lambda name: name == 'rohm_status')
    with led.installed(lib, patch_torch=False):
        _fwd(lib, current, 0x10, None, None, 0x9000)
        current[0] = 0x10
        assert lib.rohm_status(None, C.c_void_p(0x9000), 64, C.c_void_p(0x10)) == -9       # the return code passes through
        _fwd(lib, current, 0x20, None, None, 0x9000)
    found = RE.conflicts(led.entries)
    # the forward is ordered before the other stream's call by the status read; the status read itself (it writes ws: it clears the
    # word) is not
    assert [(a['function'], b['function']) for a, b, *_ in found] == [('rohm_status', 'rohm_fwd')]
    assert [e['waits'] for e in led.calls()] == [False, True, False]


def test_a_wait_that_overlaps_a_call_in_host_time_orders_nothing():
    """Hand-made entries: thread B's call returns while thread A's device synchronisation is still running."""
    call = lambda stream, enter, leave: dict(kind='call', function='rohm_fwd', thread=stream, stream=stream, handle=None, enter=enter,
                                             leave=leave, writes=[('ws', 0x9000, 0x9040)], reads=[], waits=False, deferred=False, rc=0)
    sync = lambda enter, leave: dict(kind='sync', stream=None, enter=enter, leave=leave)
    a, b = call(0x10, 1, 2), call(0x20, 6, 7)
    assert RE.conflicts([a, sync(3, 5), b]) == []                                # A returned, the wait ran, B was entered
    assert len(RE.conflicts([call(0x10, 1, 4), sync(3, 5), b])) == 1             # the wait began before A had returned
    assert len(RE.conflicts([a, call(0x20, 4, 7), sync(3, 5)])) == 1             # B was entered before the wait ended
    assert len(RE.conflicts([call(0x10, 1, 5), call(0x20, 2, 4)])) == 1          # two calls inside each other (two threads)
    assert RE.ordered(a, b, [a, sync(3, 5), b]) and not RE.ordered(b, a, [a, sync(3, 5), b])
    assert len(RE.conflicts([a, sync(3, 5), b], host_order=False)) == 1          # ... unless no wait is taken for an ordering
    assert len(RE.report([a, sync(3, 5), b], host_order=False)) == 1 and RE.report([a, sync(3, 5), b]) == []


def test_a_function_with_two_buffers_and_null_optional_outputs():
    led, current, lib = _ledger()
    with led.installed(lib, patch_torch=False):
        current[0] = 0x10
        lib.rohm_two(None, C.c_void_p(0x5000), C.c_size_t(256), C.c_void_p(0x6000), 128, C.c_void_p(0x10))
        current[0] = 0x20
        lib.rohm_two(None, C.c_void_p(0x5100), 256, None, 0, C.c_void_p(0x20))           # no scratch: NULL carries no range
        lib.rohm_two(None, C.c_void_p(0x7000), 0, C.c_void_p(0x6040), 64, C.c_void_p(0x20))      # a buffer of 0 bytes carries none either
    first, second, third = led.calls()
    assert first['writes'] == [('saved', 0x5000, 0x5100), ('scratch', 0x6000, 0x6080)]
    assert second['writes'] == [('saved', 0x5100, 0x5200)] and third['writes'] == [('scratch', 0x6040, 0x6080)]
    found = RE.conflicts(led.entries)
    assert [(wn, on, lo, hi) for _, _, wn, on, lo, hi in found] == [('scratch', 'scratch', 0x6040, 0x6080)]      # `saved` only touches


def test_a_deferred_call_is_logged_now_and_made_later():
    led, current, lib = _ledger(defer={'rohm_status'}, waits=lambda name: name == 'rohm_status')
    with led.installed(lib, patch_torch=False):
        current[0] = 0x10
        assert lib.rohm_status(None, C.c_void_p(0x9000), 64, C.c_void_p(0x10)) == 0 and lib.seen == []
        (e,) = led.calls()
        assert e['deferred'] and not e['waits'] and e['rc'] == 0                          # it has not waited: it orders nothing
        assert led.run_deferred() == [('rohm_status', -9)] and lib.seen == ['status'] and led.run_deferred() == []


def test_tensor_addresses_carry_their_extent_while_the_ledger_is_installed():
    led, current, lib = _ledger(synchronize=None)
    t = torch.zeros(4, 5)
    with led.installed(lib):
        assert t.data_ptr() and led.sizes == {}                                           # host tensors are not device memory
    assert 'data_ptr' not in vars(torch.Tensor)
    noted = []
    led = RE.Ledger(RE.abi_operands(SAMPLE), current_stream=lambda: 0, synchronize='note')
    led.note_sync = lambda stream, wait: noted.append(stream) or wait()
    real = torch.cuda.synchronize
    with led.installed(lib):
        assert torch.cuda.synchronize is not real
    assert torch.cuda.synchronize is real and 'synchronize' in vars(torch.cuda.Stream)
    led = RE.Ledger(RE.abi_operands(SAMPLE), current_stream=lambda: 0, synchronize='skip')
    with led.installed(lib):
        assert torch.cuda.synchronize() is None                                           # turned into nothing: no device is touched
    assert torch.cuda.synchronize is real


def test_two_threads_log_into_one_ledger():
    led, _, lib = _ledger()
    led.current_stream = lambda: {'reentrancy-0': 0x10, 'reentrancy-1': 0x20}[threading.current_thread().name]
    workers = RE.Workers()

    def job(stream, ws):
        def run():
            for _ in range(50):
                lib.rohm_fwd(None, None, None, None, C.c_void_p(ws), 64, C.c_void_p(stream))
            return threading.get_ident()
        return run
    with led.installed(lib, patch_torch=False):
        ids = workers.run([job(0x10, 0x9000), job(0x20, 0xA000)], timeout=20.0)
        assert RE.conflicts(led.entries) == []
        again = workers.run([job(0x10, 0x9000), job(0x20, 0x9020)], timeout=20.0)
    assert ids == again and ids[0] != ids[1] and threading.get_ident() not in ids         # the same two threads, kept
    calls = led.calls()
    assert len(calls) == 200 and {e['thread'] for e in calls} == set(ids) and led.streams_of() == {'rohm_fwd': {0x10, 0x20}}
    ticks = sorted(t for e in calls for t in (e['enter'], e['leave']))
    assert ticks == list(range(1, 401))                                                   # one counter, no tick handed out twice
    assert RE.conflicts(led.entries) and all(c[4:] == (0x9020, 0x9040) for c in RE.conflicts(led.entries))


# ---- the worker threads ------------------------------------------------------------------------------------------------------------
def test_the_workers_meet_at_a_barrier_hand_back_exceptions_and_stop_after_a_timeout():
    workers, met = RE.Workers(), []

    def arrive(i):
        def run():
            met.append((i, time.perf_counter()))
            return i * 10
        return run
    assert workers.run([arrive(0), arrive(1)], timeout=20.0) == [0, 10]
    assert sorted(i for i, _ in met) == [0, 1]

    def broken():
        raise ValueError('the job failed')
    with pytest.raises(ValueError, match='the job failed'):
        workers.run([arrive(0), broken], timeout=20.0)
    assert workers.run([arrive(0), arrive(1)], timeout=20.0) == [0, 10] and not workers.hung      # an exception is not a hang
    release = threading.Event()
    with pytest.raises(RE.WorkerTimeout, match='has not returned after 0.2 s'):
        workers.run([arrive(0), lambda: release.wait(30.0)], timeout=0.2)
    assert workers.hung
    with pytest.raises(RE.WorkerTimeout, match='nothing more is started'):
        workers.run([arrive(0), arrive(1)], timeout=20.0)
    release.set()


# ---- device intervals --------------------------------------------------------------------------------------------------------------
def test_the_overlap_of_two_device_intervals():
    elapsed = lambda x, y: y - x                                  # stand-in events: their device time in milliseconds
    assert RE.overlap_ms((10.0, 20.0), (15.0, 30.0), elapsed) == 5.0
    assert RE.overlap_ms((15.0, 30.0), (10.0, 20.0), elapsed) == 5.0
    assert RE.overlap_ms((10.0, 30.0), (15.0, 20.0), elapsed) == 5.0
    assert RE.overlap_ms((10.0, 20.0), (20.0, 30.0), elapsed) == 0.0          # one after the other: nothing shared
    assert RE.overlap_ms((10.0, 20.0), (25.0, 30.0), elapsed) == -5.0


# ---- the tables --------------------------------------------------------------------------------------------------------------------
def test_every_exemption_quotes_a_sentence_of_the_header_or_names_a_case():
    import test_gpu_bounds as B
    import test_gpu_stale_memory as G
    prose = SO.header_prose()
    waiting = RE.waiting_calls()
    assert set(waiting) == {'rohm_posenet_exchange_status', 'rohm_trajnet_sample_loop', 'rohm_track_resample', 'rohm_floor_hypotheses'}
    assert all(sentence in prose for sentence in waiting.values())
    for key, (reason, sentence) in RE.NOT_TOGETHER.items():
        assert len(reason) > 40 and len(sentence) > 40 and sentence in prose, key
        assert any(key in name for name in B.ALL), key
    assert 'tests/test_gpu_reentrancy.py holds every entry point to this' in prose
    # the pairs that are not run: the stream-K head's one case and every clip-resident loop
    skipped = sorted(name for name in B.ALL if RE.not_together(name))
    assert skipped == sorted(['output_process[B32]'] + [n for n in G.HANDLES if 'resident 1' in n]) and len(skipped) == 8
    assert RE.not_together('trajnet_loop[TrajNet, resident 0, B1, T16, 4 steps]') is None
    # every function those pairs call is still run on two streams by a pair that is: the loop in its launch-per-layer form, the head
    # on plain tiles
    assert any('resident 0' in n for n in G.HANDLES) and 'output_process[B3]' in G.CASES
    assert set(RE.THREAD_EXEMPT) <= set(G.CASES) and all(len(why) > 40 for why in RE.THREAD_EXEMPT.values())
    for f, families in RE.DEFERRED_STATUS.items():
        assert f in waiting and all(any(G.family(n) == fam for n in G.HANDLES) for fam in families)
    assert RE.R == 8
