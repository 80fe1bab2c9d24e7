"""GPU: calls are re-entrant across streams and host threads given distinct workspaces, and the Python bindings hand out distinct
workspaces (include/rohm_hip.h, "Conventions": "calls are re-entrant across streams given distinct workspaces").

The other sentences of that block have a registry-wide module each (tests/test_gpu_stale_memory.py, test_gpu_bounds.py,
test_gpu_stream_order.py, test_gpu_graph_replay.py); they all run one caller at a time.  Memory that two callers share is exactly what
tests/test_gpu_stream_order.py lists as unseen ("a stray launch ... that reads only weights or handle-owned tables and writes
handle-owned memory"), and a run with two callers in flight is what makes it visible.  Here every case of that registry (imported, not
copied: `G.CASES`, `G.HANDLES`, `B.ALL`, `B._base`, `stale_memory.differences`) runs as a PAIR:

  (1) THE LEDGER (tests/reentrancy.py; needs no race to happen).  For the duration of a pair the stream-taking `rohm_*` functions of
      the loaded library are recording wrappers: thread, stream, handle, and the address range of every buffer operand, classed by the
      header's `const` as read or written.  Two calls on different streams with no host-visible ordering between them (a device or
      stream synchronisation, a call the header documents as waiting) may not share a range that one of them writes.  The check is
      also made with no wait taken for an ordering: what two streams were handed in one run is held to be distinct.
  (2) TWO STREAMS, ONE HOST THREAD, RELEASED TOGETHER.  A case with a cached handle (`G.HANDLES`): one handle `h`; call(h, 0) and
      call(h, 1) alone on the default stream, twice each (bit-equal: the baselines); then call(h, 0) R = 8 times on one side stream
      and call(h, 1) 8 times on the other, both streams waiting for ONE event behind a gate (a delay kernel, stream_order.Gates) on a
      third stream.  Every other case: the case itself on both sides, once.  While the host queues, every upload goes through
      stream_order.DeferredInputs (the registry's `_d`, torch.tensor(..., device=), .to(<the GPU>) of a host tensor: a blocking copy
      would sit out the gate), torch.cuda.synchronize is nothing, and the closing status read of the PoseNet cases
      (rohm_posenet_exchange_status, which waits) is deferred until the gate is open and must then return ROHM_OK.  Every output of
      every run equals its baseline BIT FOR BIT.  For a `HANDLES` pair the run counts only if the two device intervals (an event in
      front of each side's work, one behind its last run, `elapsed_time` across the streams) intersect: a side whose work was queued
      after the gate had run out has its head stamped late.  Whether the gate was still closed when the last call was queued is
      recorded.  For the single cases the overlap is recorded and not required (many wait inside: .item(), a host check), and their
      gate is at most 100 ms.
  (3) TWO HOST THREADS, one stream each, one handle, released by a threading.Barrier (reentrancy.Workers: two threads kept for the
      whole module, joined with a 60 s timeout; after a timeout every later test fails before it touches the GPU).  ctypes releases
      the GIL, so the library is entered twice at once.  No `_d` patch and no poisoning allocator is active; the ledger's wrappers are
      installed before the threads are released and removed after they are joined.  Bit equality with the baselines, the ledger, and
      for `HANDLES` pairs intersecting device intervals.  Plus: rohm_last_error per thread; two threads creating handles at once;
      TrajControl's launch-per-layer loop from two threads and from two caller streams of one thread.
  (4) THE CHECK CAN FAIL (run first; it picks the side streams).  A fake entry point made of torch ops, y = (x * 2 kept in `scratch`)
      + 1 with a 2 ms delay between the two steps: with ONE scratch for both sides the ledger names it (`writes `scratch``, 16384
      bytes) and, released together, at least one side's y is wrong whichever product lands last; with a scratch per side both checks
      pass.  With few hardware queues two streams may share one and then run one after the other: up to 8 pairs of
      torch.cuda.Stream() are tried and the module fails if none shows the wrong y.  On MI355X with 4 hardware queues the FIRST pair did.

Pairs that are not run this way (tables in tests/reentrancy.py, each quoting the header):
  * `TWO_THREADS_ONLY`: posenet_guided (the guided step polls rohm_posenet_exchange_status after its forward and acts on the answer),
    track_resample (rohm_track_resample), floor (rohm_floor_hypotheses): calls the header documents as waiting cannot be queued behind
    a closed gate from one thread.  They run in (3); their ledger is the order-blind one.
  * `NOT_TOGETHER`, decided from the code before any run.  Which launches let workgroups meet through L2, and do two of them fit on
    256 CUs at the registry's shapes?
      - the LayerNorm-carrying GEMMs (gemm_f32.hip launch_one, EPI_BIAS_RES_LN): grid = row tiles rounded up to 8 x column tiles, one
        workgroup per CU (84 KiB of LDS).  PoseNet at B <= 3 (3 row tiles): 8 x 8 = 64 workgroups, 8 per XCD, 24 of them with work;
        gemm_res_layernorm[288x512x64] and [144x1024x32]: 64 each.  Two launches: 128 of 256 CUs, 16 of 32 per XCD.  THEY FIT: run.
      - the `chain` / `stack` forms under ROHM_POSENET_CHAIN_ANY (encoder_chain.hip): groups8 x 8 parts = 64 persistent workgroups at
        B <= 3, one per CU.  Two launches: 128.  THEY FIT: run.  A set error word is a failure: the deferred status read must return 0.
      - the stream-K head (kSkWorkgroups = 256, one per CU): PoseNet at B <= 3 has 5 / 10 / 15 output tiles, no multiple of 8, and
        takes plain tiles (gemm_sk_plan); only output_process[B32] is stream-K.  Two launches ask for 512 one-per-CU slots: THEY CANNOT
        FIT.  Not run; its entry point is run on two streams by output_process[B3].
      - the clip-resident TrajNet step (trajnet_resident.hip: 8 XCDs x 32 workgroups, all 32 of an XCD meet after every layer): 512
        slots for two.  THEY CANNOT FIT.  The seven `resident 1` cases are not run; the same loop runs in its `resident 0` form.
    include/rohm_hip.h says so next to the re-entrancy sentence since this module.  Each pair runs once: no retry anywhere.
  * `THREAD_EXEMPT` (reasons of the CASE, not of the library; they run in (2)): clips_repr (patches torch's allocators itself),
    posenet_train with dropout 0.1 (draws its seed from torch's process-wide CPU generator).
  * control calls that the header says must not race with launches are not exercised: rohm_posenet_set_exchange,
    rohm_posenet_inject_exchange_fault, rohm_posenet_set_stack_timeline, rohm_trajnet_tune, the profiler.

Coverage, computed from stream_order.abi_stream_functions(): all 78 entry points with a stream parameter were called on both streams
of at least one pair; STREAM_PAIR_EXEMPT is empty.  The four waiting calls were all entered from two threads.

Findings:
  * rohm_amd/body_model.py kept ONE guidance workspace and ONE skinning workspace per SMPL-X handle, whatever the stream
    (`_NativeSMPLX.workspace`, `lbs_workspace`), and `native_for` caches that handle on the body model; `lbs_workspace` dropped the old
    block when it grew, while another stream's launch could still be using it.  With that binding (the parent commit's) this module
    fails for guidance_skating, guidance_skating_split, guidance_proj2d, posenet_guided and all eight smplx_forward pairs:
      guidance_skating[B2, T50]: rohm_guidance_skating_grad on stream 0x629e2ae4b1f0 (thread 138873414895424) writes `ws` and
        rohm_guidance_skating_grad on stream 0x629e2ab5ce30 (thread 138873414895424) writes `ws`: shared range [0x7e44704f1a00,
        0x7e44704f4128), 10024 bytes, no host-visible ordering between the two calls ... and 61 more
      smplx_forward[mfma, N1, verts]: rohm_smplx_forward on stream 0x629e2ae4b1f0 ... writes `ws` and rohm_smplx_forward on stream
        0x629e2ab5ce30 ... writes `ws`: shared range [0x7e444954e200, 0x7e4449691200), 1323008 bytes ... and 61 more
    and the numbers were wrong, not only the arguments: guidance_skating caller 0, runs 3 - 7, grad element 2151 0.1456 for -0.0262;
    smplx_forward[mfma, N17, joints only] caller 0, joints element 0 2.2551 / 1.7168 for 2.0551; every smplx_forward pair differed
    from both threads as well.  (posenet_guided's two threads happened to wait between every two guidance calls in that run: its
    timing-aware ledger was clean, which is why the order-blind check exists; with it: `ws`, 27880 bytes, from both threads.)  Fixed: both workspaces are kept per HIP stream, as
    `_NativePoseNet.workspace`; a stream's buffer is replaced only by a call on that stream, and torch's allocator hands a block back
    to the stream it was allocated on.  After the fix all of them pass, and tests/test_gpu_stale_memory.py (carried state),
    test_gpu_bounds.py, test_gpu_stream_order.py, test_gpu_graph_replay.py, test_gpu_guidance.py, test_gpu_rederive.py and
    test_gpu_posenet.py pass unchanged (527 tests).
  * `_NativePoseNet.workspace` / `_NativeTrajNet.workspace` iterated over their cache dict while another thread could insert into it
    ("dictionary changed size during iteration"): they iterate over a snapshot of the keys now.  Seen by reading.
  * One thread, two caller streams, TrajControl's launch-per-layer loop: both calls share the thread's one control stream, which runs
    up to a step ahead of its caller.  Results are bit-identical, and the two sides do start together, but the second caller's
    branches queue behind all of the first caller's: measured from the END of each side's first loop the two sides do not intersect
    (-1.97 / -2.10 / -2.26 ms at B1 T16 / B9 T48 / B9 T144, 8 loops of 4 steps each), where every other `HANDLES` pair does.  Correct,
    documented (one control stream per host thread), and slower than two threads would be.  Left as it is.
  * rohm_amd.guidance.guide_2d_projection uploads the dataset's camera (cam_R, cam_t) from host memory at every call: a blocking copy
    per guided step, invisible to tests/test_gpu_stream_order.py (which holds the `rohm_*` calls, not the wrappers).  It is what first
    drained this module's gate.  Left as it is (a cache would have to notice a camera that changes between recordings).
  * Read and judged, not instrumented: the `static bool attr_set[...]` / `lds_set` flags in front of hipFuncSetAttribute
    (gemm_f32.hip:821, encoder_chain.hip:922 / 980, attention_f32.hip, lbs.hip:550, clips.hip, trajnet_resident.hip:837, gemm_pp.hip)
    are written without synchronisation.  Two threads that both find a flag clear both set the same attribute to the same value and
    both set the flag; a thread that finds it set launches through the runtime's own lock, after the attribute call that preceded
    the store.  Formally a data race on a bool, in effect idempotent.  In this module every kernel has been launched by the baselines
    before two threads meet it.  The thread_local control stream of trajnet.hip is never destroyed: a process that starts many
    short-lived threads which each run a TrajControl loop leaves a stream and five events behind per thread (this module keeps two
    threads for that reason).
  * Nothing else: rohm_last_error is per thread (200 refusals next to 200 good calls), handles created side by side compute what
    handles created alone compute (PoseNet `layer` form: the per-handle tag salt; TrajNet; SMPL-X), no exchanging pair set its error
    word, and no other binding hands two streams one buffer (ops.*, rig, fit, fit_views, multiview, render, occlusion allocate per call).

Numbers (MI355X, GPU_MAX_HW_QUEUES = 4).  R = 8.  86 cases: 75 gated pairs (37 of them `HANDLES` pairs) and 75 threaded pairs (38); 8 are
not run together, 3 run from two threads only, 3 from one thread only.  1036 logged calls in the gated runs, 1118 in the threaded ones.
Gates: four times the host time of the runs alone plus 30 ms, 33 ms .. 956 ms (capped at 1 s; 100 ms for the single cases), 10.9 s in
all; queuing behind a closed gate took up to 2.6 times the host time of the same runs alone.  53 of 75 gates were still closed when
the last call was queued: 36 of the 37 `HANDLES` gates -- trajnet_loop[TrajControl, resident 0, B1, T16] filled the queue in two runs
of three (queued in 221 ms of a 216 ms gate, overlap 0.46 ms) -- and 17 of the 38 single cases.  Device overlap of the `HANDLES` pairs,
gated: 0.34 .. 25.3 ms, median 2.9 ms; threaded: 3.2 .. 101.3 ms, median 15.1 ms.  57 of 75 gated pairs and all 75 threaded pairs
overlapped (the 18 that did not are single cases that wait inside).  The fake pair: first pair of streams, 2.40e6 delay units per ms.
Wall time of the whole module, 237 tests, run alone: 29.7 s (the slowest test 1.5 s; 27.5 s with gates of 2.5 times the host time);
within the whole suite its baselines are shared with tests/test_gpu_bounds.py.  profiles/reentrancy.json holds the per-pair figures.

What stays unseen -- nobody should take it for covered:
  * more than two concurrent callers; two devices in one process (one handle per device, a second device's control stream);
  * interleavings that the two release schemes cannot force: the gate releases both queues at one instant and the barrier both threads,
    but which kernels then meet on the device is the hardware's choice, run once;
  * device memory reached through a host TABLE of pointers (rohm_adamw_step, rohm_grad_norm, the `grads` of
    rohm_trajnet_train_backward): the ledger sees the table, not what it points to; handle-owned memory (weights, tables): the ledger
    sees the handle, not its allocations -- two callers of one handle are held to bit equality only;
  * host waits the ledger cannot see (.item(), a blocking copy) order nothing in it: it errs towards reporting;
  * the pairs of NOT_TOGETHER, by decision; the control calls the header excludes; a sanitizer's view of the host-side races above.
Reference work: none (bit equality with the same call made alone)."""
import contextlib
import ctypes as C
import json
import os
import threading
import time

import pytest
import torch

import reentrancy as RE
import stale_memory as SM
import stream_order as SO
import test_gpu_bounds as B
import test_gpu_stale_memory as G
from helpers import seeded

pytestmark = pytest.mark.gpu
DEV = G.DEV
ALL = B.ALL                                     # the registry's cases and EXTRA of tests/test_gpu_bounds.py
R = RE.R                                        # calls queued per side for a case with a cached handle (every other case: one)
OPERANDS = RE.abi_operands()
STREAM_AT = SO.abi_stream_functions()
JOIN_TIMEOUT = 60.0                             # seconds a worker thread may take before the module gives up on it
MAX_STREAM_PICKS = 8
MIN_GATE, MAX_GATE, MAX_PLAIN_GATE = 0.030, 1.0, 0.100       # seconds
FAKE_DELAY_MS = 2.0
FAKE_GATE = 0.100
GATE_MARGIN = 4.0                               # queuing behind a closed gate took up to 2.6 times the host time of the runs alone
WORKERS = RE.Workers()
_REAL_SYNC = torch.cuda.synchronize

RUN = sorted(n for n in ALL if not RE.not_together(n))                          # pairs that may be in flight together
GATED = [n for n in RUN if G.family(n) not in RE.TWO_THREADS_ONLY]              # ... and can be queued behind a closed gate
THREADED = [n for n in RUN if n not in RE.THREAD_EXEMPT]
# stream-taking entry points that no pair puts on two streams, each with the header sentence that says why (none today)
STREAM_PAIR_EXEMPT = {}


def _alive():
    if WORKERS.hung:
        pytest.fail('a worker thread did not return from an earlier test of this module: no further GPU work is started')


def _env_for(name):
    """The environment a case sets around its call, set once around both callers (two threads must not set and restore it)."""
    for form in ('0', '1'):
        if f'resident {form}' in name:
            return SM.env(ROHM_TRAJ_RESIDENT=form)
    return contextlib.nullcontext()


def _lib():
    from rohm_amd import _lib
    return _lib.lib()


# ================================================================================================ the two sides of a pair
class _Side:
    """One caller: `fn` run `reps` times under `stream`, an event in front of its work and one behind every run."""

    def __init__(self, stream, fn, inputs=None, reps=1):
        self.stream, self.fn, self.inputs, self.reps = stream, fn, inputs, reps
        self.head = torch.cuda.Event(enable_timing=True)
        self.marks = [torch.cuda.Event(enable_timing=True) for _ in range(reps)]
        self.outs = []

    def work(self):
        with torch.cuda.stream(self.stream):
            self.head.record()
            for r in range(self.reps):
                if self.inputs is not None:
                    self.inputs.replayed = 0                     # every run asks for the recorded inputs again
                self.outs.append(SM.snapshot(self.fn()))
                self.marks[r].record()

    def interval(self):
        """The device interval of the side's work: from the event in front of it to the event behind its last run."""
        return (self.head, self.marks[-1])

    def late_interval(self):
        """From the END of the first run to the end of the last (one run: as interval()).  Behind a gate the head is stamped when the
        gate opens, whatever follows it; this narrower interval starts at the first stamp that finished work has earned."""
        return (self.marks[0], self.marks[-1]) if self.reps > 1 else self.interval()

    def differences(self, base):
        out = []
        for r, got in enumerate(self.outs):
            out += [(r, label, d) for label, d in SM.differences(got, base)]
        return out


@contextlib.contextmanager
def _uploads_through(d):
    """Every upload goes through `d` (stream_order.DeferredInputs.record / .replay): the registry's `_d`, `torch.tensor(...,
    device=<the GPU>)` (the timesteps of the PoseNet / TrajNet cases) and `.to(<the GPU>)` of a host tensor (what the wrappers upload
    themselves: the camera of the 2-D guidance, the statistics, a module's parameters).  A blocking upload would sit out the gate.
    One host thread only."""
    real_tensor, real_to, inside = torch.tensor, torch.Tensor.to, [False]

    def through(t):
        inside[0] = True                        # (`d` uploads with .to itself)
        try:
            return d(t)
        finally:
            inside[0] = False

    def gpu(dev):
        return isinstance(dev, (str, torch.device)) and torch.device(dev).type == 'cuda'

    def tensor(*a, **k):
        if not inside[0] and gpu(k.get('device')):
            return through(real_tensor(*a, **{key: v for key, v in k.items() if key != 'device'}))
        return real_tensor(*a, **k)

    def to(self, *a, **k):
        if not inside[0] and self.device.type == 'cpu' and gpu(k.get('device', a[0] if a else None)):
            dtype = k.get('dtype', next((x for x in a if isinstance(x, torch.dtype)), None))
            host = self.detach() if dtype is None else real_to(self.detach(), dtype)
            return through(host.contiguous())
        return real_to(self, *a, **k)
    with pytest.MonkeyPatch.context() as m:
        m.setattr(G, '_d', through)
        m.setattr(torch, 'tensor', tensor)
        m.setattr(torch.Tensor, 'to', to)
        yield


def _overlaps(sides, error):
    if error is not None:
        return dict(overlap_ms=None, late_overlap_ms=None)
    return dict(overlap_ms=RE.overlap_ms(sides[0].interval(), sides[1].interval()),
                late_overlap_ms=RE.overlap_ms(sides[0].late_interval(), sides[1].late_interval()))


def _released_together(h, sides, lib_obj, operands, length, waits=lambda f: False, defer=()):
    """One host thread: a gate of `length` seconds on the third stream, both sides wait for the event behind it, side 0's runs are
    queued, then side 1's; the gate opens.  -> dict(ledger, overlap_ms, closed, queued, status, error)"""
    led = RE.Ledger(operands, waits=waits, defer=defer, synchronize='skip')
    gates = SO.Gates(h['gate'], length, h['delay'], h['rate'])
    error, closed, queued, t0 = None, None, None, time.perf_counter()
    try:
        with led.installed(lib_obj):
            gates.arm()
            for s in sides:
                s.stream.wait_event(gates.event)
            for s in sides:
                with _uploads_through(s.inputs.replay) if s.inputs is not None else contextlib.nullcontext():
                    s.work()
            queued = time.perf_counter() - t0
            closed = gates.closed()
    except Exception as e:                      # kept for the pair's own test
        error = e
    finally:
        _REAL_SYNC()
    status = led.run_deferred() if error is None else []
    _REAL_SYNC()
    return dict(ledger=led, closed=closed, queued=queued, gate=length, status=status, error=error, **_overlaps(sides, error))


def _from_two_threads(sides, lib_obj, operands, name='', waits=lambda f: False):
    """Two host threads released by a barrier, one side each.  No `_d` patch and no poisoning allocator is active."""
    led = RE.Ledger(operands, waits=waits, synchronize='note')
    error = None
    try:
        with _env_for(name), led.installed(lib_obj):
            WORKERS.run([s.work for s in sides], JOIN_TIMEOUT)
    except RE.WorkerTimeout:
        raise                                   # nothing more is started, not even a synchronisation
    except Exception as e:
        error = e
    _REAL_SYNC()
    return dict(ledger=led, error=error, **_overlaps(sides, error))


# ================================================================================================ the check can fail: a fake pair
class _FakeLib:
    """A fake entry point made of torch ops: y = (x * 2, kept in `scratch`) + 1, with a delay between the two steps."""

    def __init__(self, delay):
        self.delay, self.tensors = delay, {}

    def arg(self, t):
        self.tensors[t.data_ptr()] = t
        return C.c_void_p(t.data_ptr())

    def rohm_fake_scale_add(self, x, y, scratch, scratch_bytes, stream):
        x, y, tmp = (self.tensors[RE.address(p)] for p in (x, y, scratch))
        torch.mul(x, 2.0, out=tmp)
        self.delay()
        torch.add(tmp, 1.0, out=y)
        return 0


_FAKE_OPERANDS = {'rohm_fake_scale_add': dict(stream=4, handle=None, operands=[('x', 0, None, False), ('y', 1, None, True),
                                                                                ('scratch', 2, 3, True)])}


def _fake_pair(h, streams, shared, threads=False):
    """-> (result, [differences of side 0, of side 1])"""
    from rohm_amd._lib import stream_ptr
    fake = _FakeLib(lambda: h['delay'](h['rate'] * FAKE_DELAY_MS))
    xs = [seeded(1, 4096).to(DEV), seeded(2, 4096).to(DEV)]
    tmps = [torch.empty(4096, device=DEV)] * 2 if shared else [torch.empty(4096, device=DEV), torch.empty(4096, device=DEV)]
    base = [[('y', x * 2.0 + 1.0)] for x in xs]
    _REAL_SYNC()

    def caller(x, tmp):
        def fn():
            y = torch.empty_like(x)
            fake.rohm_fake_scale_add(fake.arg(x), fake.arg(y), fake.arg(tmp), tmp.numel() * 4, stream_ptr())
            return [('y', y)]
        return fn
    sides = [_Side(s, caller(x, tmp)) for s, x, tmp in zip(streams, xs, tmps)]
    if threads:
        r = _from_two_threads(sides, fake, _FAKE_OPERANDS)
    else:
        r = _released_together(h, sides, fake, _FAKE_OPERANDS, FAKE_GATE)
    assert r['error'] is None, r['error']
    return r, [s.differences(b) for s, b in zip(sides, base)]


_HARNESS = {}


def _harness():
    """The gate's stream and the two side streams, picked by the fake pair with one shared scratch: with few hardware queues two
    streams may share one, and two sides that share a queue run one after the other.  -> dict(gate, a, b, delay, rate, attempt)"""
    if not _HARNESS:
        delay, guess = SO.torch_delay()
        gate = torch.cuda.Stream()
        rate = SO.calibrate(delay, guess, gate)
        _HARNESS.update(gate=gate, a=None, b=None, delay=delay, rate=rate, attempt=None, tried=[], keep=[])
        _fake_pair(_HARNESS, (gate, gate), shared=False)        # (the first launch of a kernel loads its code: not behind a gate)
        for attempt in range(1, MAX_STREAM_PICKS + 1):
            a, b = torch.cuda.Stream(), torch.cuda.Stream()
            _HARNESS['keep'] += [a, b]
            r, diffs = _fake_pair(_HARNESS, (a, b), shared=True)
            seen = dict(bits=bool(diffs[0] or diffs[1]), ledger=bool(RE.conflicts(r['ledger'].entries)), closed=r['closed'],
                        overlap_ms=round(r['overlap_ms'], 3))
            _HARNESS['tried'].append(seen)
            if seen['bits']:
                _HARNESS.update(a=a, b=b, attempt=attempt)
                break
    assert _HARNESS['a'] is not None, (f'no pair of {MAX_STREAM_PICKS} runs its sides at the same time: {_HARNESS["tried"]}; the rest of the '
                                       f'module would prove nothing')
    return _HARNESS


def test_the_fake_pair_with_one_shared_scratch_fails_both_checks_and_picks_the_streams():
    """Each side: tmp = x * 2, a delay, y = tmp + 1, with `tmp` one tensor for both.  Released together both products are written before
    either sum is taken: at least one side's y is wrong, whichever product lands last.  No library code runs."""
    h = _harness()
    print(f'side streams: attempt {h["attempt"]} of {MAX_STREAM_PICKS}, {h["rate"]:.0f} delay units per ms, tried {h["tried"]}')
    seen = h['tried'][-1]
    assert seen['bits'] and seen['ledger'] and seen['closed'] and seen['overlap_ms'] > 0.0
    r, diffs = _fake_pair(h, (h['a'], h['b']), shared=True)
    assert diffs[0] or diffs[1]
    text = RE.report(r['ledger'].entries)
    assert len(text) == 1 and 'rohm_fake_scale_add' in text[0] and 'writes `scratch`' in text[0] and '16384 bytes' in text[0], text


def test_the_fake_pair_with_a_scratch_per_side_passes_both_checks():
    h = _harness()
    r, diffs = _fake_pair(h, (h['a'], h['b']), shared=False)
    assert diffs == [[], []] and RE.report(r['ledger'].entries) == [] and r['closed'] and r['overlap_ms'] > 0.0
    assert r['ledger'].streams_of() == {'rohm_fake_scale_add': {int(h['a'].cuda_stream), int(h['b'].cuda_stream)}}


def test_the_fake_pair_from_two_threads():
    """The ledger reports the shared scratch whatever the timing; with a scratch per side both checks pass."""
    _alive()
    h = _harness()
    r, _ = _fake_pair(h, (h['a'], h['b']), shared=True, threads=True)
    text = RE.report(r['ledger'].entries)
    assert len(text) == 1 and 'writes `scratch`' in text[0], text
    r, diffs = _fake_pair(h, (h['a'], h['b']), shared=False, threads=True)
    assert diffs == [[], []] and RE.report(r['ledger'].entries) == []
    assert len({e['thread'] for e in r['ledger'].calls()}) == 2


# ================================================================================================ baselines
_BASE = {}


def _base(name):
    """Alone, on the default stream, twice each: the outputs both callers must reproduce, the inputs they upload (recorded in the first
    run), the functions the case calls and the host seconds of one run.  A case with a cached handle: call(h, 0) and call(h, 1) on one
    handle `h`; every other case: the case itself for both callers (tests/test_gpu_bounds.py::_base)."""
    if name not in _BASE:
        led = RE.Ledger(OPERANDS, synchronize=None)
        if name in G.HANDLES:
            make, call = G.HANDLES[name]
            with _env_for(name):
                handle = make()
                fns = [lambda k=k: call(handle, k) for k in (0, 1)]
                bases, inputs, seconds = [], [], 0.0
                for fn in fns:
                    first = SM.snapshot(fn())                    # (the first call on a handle fills the binding's caches: not recorded)
                    _REAL_SYNC()
                    rec = SO.DeferredInputs(DEV)
                    t0 = time.perf_counter()
                    with _uploads_through(rec.record), led.installed(_lib()):
                        second = SM.snapshot(fn())
                    _REAL_SYNC()
                    seconds += time.perf_counter() - t0
                    diff = SM.differences(second, first)
                    assert not diff, f'{name}: two runs alone differ: {diff[:3]}'
                    bases.append(first)
                    inputs.append(rec)
            reps = R
        else:
            fn = ALL[name]
            base, repeatable = B._base(name)
            assert repeatable, f'{name}: two runs alone differ (rule (b) of tests/test_gpu_stale_memory.py: no case needs it on MI355X)'
            rec = SO.DeferredInputs(DEV)
            t0 = time.perf_counter()
            with _uploads_through(rec.record), led.installed(_lib()):
                third = SM.snapshot(fn())
            _REAL_SYNC()
            seconds = 2.0 * (time.perf_counter() - t0)
            diff = SM.differences(third, base)
            assert not diff, f'{name}: recording the inputs changes the run: {diff[:3]}'
            twin = SO.DeferredInputs(DEV)
            twin.recorded = list(rec.recorded)
            fns, bases, inputs, reps = [fn, fn], [base, base], [rec, twin], 1
        for rec in inputs:
            rec.stage()
        _REAL_SYNC()
        _BASE[name] = dict(fns=fns, bases=bases, inputs=inputs, reps=reps, seconds=seconds, functions=set(led.streams_of()))
    return _BASE[name]


def _summary(name, r, sides, bases):
    led = r['ledger']
    return dict(error=r['error'], diffs=[s.differences(b) for s, b in zip(sides, bases)] if r['error'] is None else None,
                report=RE.report(led.entries), report_any_order=RE.report(led.entries, host_order=False), streams=led.streams_of(), threads={e['thread'] for e in led.calls()},
                calls=len(led.calls()), overlap_ms=r['overlap_ms'], late_overlap_ms=r['late_overlap_ms'], closed=r.get('closed'), queued=r.get('queued'), gate=r.get('gate'),
                status=r.get('status', []), waited=sorted({e['function'] for e in led.calls() if e['waits']}), reps=sides[0].reps)


# ================================================================================================ two streams, one host thread
_GATED, _THREADED = {}, {}


def _gated(name):
    if name not in _GATED:
        h, b = _harness(), _base(name)
        fam = G.family(name)
        sides = [_Side(s, fn, rec, b['reps']) for s, fn, rec in zip((h['a'], h['b']), b['fns'], b['inputs'])]
        # long enough for the host to queue both sides (measured alone, waits included: an over-estimate); a case without a cached
        # handle need not overlap and may wait inside: its gate is kept short
        length = min(MAX_GATE if name in G.HANDLES else MAX_PLAIN_GATE, max(MIN_GATE, GATE_MARGIN * b['reps'] * b['seconds'] + 0.030))
        defer = {f for f, fams in RE.DEFERRED_STATUS.items() if fam in fams}
        with _env_for(name):
            r = _released_together(h, sides, _lib(), OPERANDS, length, waits=lambda f: SO.may_wait(f, name), defer=defer)
        _GATED[name] = _summary(name, r, sides, b['bases'])
    return _GATED[name]


def _threaded(name):
    if name not in _THREADED:
        h, b = _harness(), _base(name)
        sides = [_Side(s, fn, None, b['reps']) for s, fn in zip((h['a'], h['b']), b['fns'])]
        r = _from_two_threads(sides, _lib(), OPERANDS, name, waits=lambda f: SO.may_wait(f, name))
        _THREADED[name] = _summary(name, r, sides, b['bases'])
    return _THREADED[name]


def _hold(name, r, what):
    if r['error'] is not None:
        raise r['error']
    bad = [(f, rc) for f, rc in r['status'] if rc != 0]
    assert not bad, f'{name}: the exchange status read after the run reports {bad}'
    for side, diff in enumerate(r['diffs']):
        assert not diff, (f'{name}: caller {side} gets another result {what}: {diff[:3]} (run, output, (first differing element, value '
                          f'here, value alone))')


@pytest.mark.parametrize('name', GATED)
def test_two_streams_released_together_compute_what_each_computes_alone(name):
    _alive()
    r = _gated(name)
    print(f'{name}: {r["calls"]} logged calls, {r["reps"]} runs per side, gate {1e3 * r["gate"]:.0f} ms, queued in '
          f'{1e3 * (r["queued"] or 0):.1f} ms, gate still closed then: {r["closed"]}, device overlap {r["overlap_ms"]} ms (from each side\'s first '
          f'run\'s end: {r["late_overlap_ms"]} ms)')
    _hold(name, r, 'when two streams are released together')
    assert not r['waited'], (f'{name}: the case makes a call the header documents as waiting ({r["waited"]}): it cannot be queued '
                             f'behind a gate and belongs in reentrancy.TWO_THREADS_ONLY')
    others = r['threads'] - {threading.get_ident()}              # (autograd runs a backward on a thread of its own)
    assert r['calls'] > 0 and (not others or G.family(name) in B.PARAMS_ON_CANVASES), r['threads']
    if name in G.HANDLES:
        # a run in which the two sides were not in flight together proves nothing.  (Whether the gate was still closed when the last
        # call was queued is printed, not required: the 16 loops of trajnet_loop[TrajControl, resident 0, B1, T16] are more launches
        # than the runtime queues behind a closed gate, the host then waits for the gate and queues the rest while the device works
        # through the backlog.  A gate that ran out EARLY shows here: the late side's head is stamped after the other side is done.)
        assert r['overlap_ms'] > 0.0, f'{name}: the two sides did not overlap on the device ({r["overlap_ms"]:.3f} ms)'


@pytest.mark.parametrize('name', RUN)
def test_two_streams_are_handed_distinct_memory(name):
    """The ledger of the pair's run (one thread; for the cases that wait, two threads): needs no race to happen."""
    _alive()
    r = _gated(name) if name in GATED else _threaded(name)
    if r['error'] is not None and not r['report']:
        raise r['error']
    assert not r['report'], f'{name}: ' + '; '.join(r['report'])
    assert not r['report_any_order'], f'{name}: ' + '; '.join(r['report_any_order'])
    both = {f for f, streams in r['streams'].items() if len(streams) >= 2}
    assert both and both == set(r['streams']), f'{name}: not every call was made on both streams: {r["streams"]}'


# ================================================================================================ two host threads
@pytest.mark.parametrize('name', THREADED)
def test_two_host_threads_compute_what_each_computes_alone(name):
    _alive()
    r = _threaded(name)
    print(f'{name}: {r["calls"]} logged calls from threads {sorted(r["threads"])}, {r["reps"]} runs per side, device overlap '
          f'{r["overlap_ms"]} ms, documented waits: {r["waited"]}')
    _hold(name, r, 'when two host threads call at once')
    assert not r['report'], f'{name}: ' + '; '.join(r['report'])
    assert r['calls'] > 0 and len(r['threads']) >= 2
    fam = G.family(name)
    if fam in RE.TWO_THREADS_ONLY:
        assert RE.TWO_THREADS_ONLY[fam] in r['waited'], (fam, r['waited'])      # the table is true: the case does make that call
    if name in G.HANDLES:
        assert r['overlap_ms'] > 0.0, f'{name}: the two threads\' work did not overlap on the device ({r["overlap_ms"]:.3f} ms)'


_CONTROL_LOOPS = [n for n in G.HANDLES if n.startswith('trajnet_loop[TrajControl, resident 0')]


@pytest.mark.parametrize('name', _CONTROL_LOOPS)
def test_the_control_loop_from_two_threads_and_from_two_streams_of_one_thread(name):
    """TrajControl's launch-per-layer loop keeps a control stream and five events per HOST THREAD (trajnet.hip side_stream).  Two
    threads: one control stream each.  One thread, two caller streams: both calls share the one control stream and its events; a wait
    takes the event's record at the time of the wait, and the shared stream only serialises the two branches."""
    _alive()
    for r, what in ((_threaded(name), 'from two threads'), (_gated(name), 'on two streams of one thread')):
        _hold(name, r, what)
        assert len(r['streams']['rohm_trajnet_sample_loop']) == 2 and r['overlap_ms'] > 0.0, (what, r['streams'], r['overlap_ms'])
    assert len(_threaded(name)['threads']) == 2 and len(_gated(name)['threads']) == 1
    assert _lib().rohm_trajnet_loop_mode() in (0, 1)


def test_last_error_is_per_thread():
    """One thread makes calls that are refused on the host before any launch (tests/test_gpu_kernel_contract.py: a LayerNorm width the
    kernel does not have), the other makes good GEMM calls after one refusal of its own (K = 48): each reads back only its own
    message, and the good calls compute what they compute alone."""
    _alive()
    from rohm_amd import _lib, ops
    h, n = _harness(), 200
    x768, g768, b768 = torch.zeros(4, 768, device=DEV), torch.ones(768, device=DEV), torch.zeros(768, device=DEV)
    a, w, bias = seeded(1, 144, 64).to(DEV), (seeded(2, 128, 64) / 8.0).to(DEV), seeded(3, 128).to(DEV)
    a48, w48, res = torch.zeros(144, 48, device=DEV), torch.zeros(128, 48, device=DEV), torch.zeros(144, 128, device=DEV)
    alone = ops.gemm(a, w, bias)
    assert SM.first_difference(ops.gemm(a, w, bias), alone) is None
    _REAL_SYNC()

    def refused():
        seen = []
        with torch.cuda.stream(h['a']):
            for _ in range(n):
                with pytest.raises(_lib.RohmHipError, match='768'):
                    ops.layernorm_(x768, g768, b768)
                seen.append(_lib.lib().rohm_last_error())
        return seen

    def good():
        seen, outs = [], []
        with torch.cuda.stream(h['b']):
            with pytest.raises(_lib.RohmHipError, match='K=48'):
                ops.gemm(a48, w48, bias, res, 2)
            own = _lib.lib().rohm_last_error()
            for _ in range(n):
                outs.append(ops.gemm(a, w, bias))
                seen.append(_lib.lib().rohm_last_error())
        return own, seen, outs
    bad_seen, (own, good_seen, outs) = WORKERS.run([refused, good], JOIN_TIMEOUT)
    _REAL_SYNC()
    assert len(bad_seen) == n and all(m and b'layernorm' in m and b'768' in m for m in bad_seen), set(bad_seen)
    assert own and b'gemm' in own and b'K=48' in own, own
    assert all(not m or (b'gemm' in m and b'layernorm' not in m) for m in good_seen), set(good_seen)
    assert all(SM.first_difference(o, alone) is None for o in outs)
    assert not bool(x768.any())                                   # refused before any launch


def test_two_threads_create_handles_at_once():
    """Two PoseNet handles with different weights created at the same moment (the layout probe's mutex, the per-handle tag salt of the
    exchanging launches), then a TrajNet handle and an SMPL-X handle alongside: the first forward of each equals that of a handle
    created alone."""
    _alive()
    from rohm_amd.body_model import native_for
    from rohm_amd.utils import synth
    dev = torch.device(DEV)

    def posenet(seed):
        net = G._make_posenet(None)
        net.load_state_dict(synth.posenet_state_dict(seed, num_layers=2), strict=False)
        return net

    def create_and_run(net, run):
        def job():
            net.native(dev)
            out = SM.snapshot(run(net))
            torch.cuda.current_stream().synchronize()
            return out
        return job

    def lbs(body):
        def job():
            nat = native_for(body, DEV)
            out = SM.snapshot(G._lbs((body, nat), 17, True))
            torch.cuda.current_stream().synchronize()
            return out
        return job
    pose_run, traj_run = (lambda net: G._pose_forward(net, 3, 143)), (lambda net: G._traj_forward(net, 9, 48))
    with SM.env(**G._POSE_ENV['layer']), SM.env(ROHM_LBS_SKIN='mfma'):
        alone = [create_and_run(posenet(21), pose_run)(), create_and_run(posenet(22), pose_run)(),
                 create_and_run(G._make_trajnet(False), traj_run)(), lbs(G._body().to(DEV))()]
        assert SM.differences(alone[0], alone[1]), 'the two PoseNets must differ'
        _REAL_SYNC()
        nets = [posenet(21), posenet(22), G._make_trajnet(False)]
        body = G._body().to(DEV)
        _REAL_SYNC()
        got = WORKERS.run([create_and_run(nets[0], pose_run), create_and_run(nets[1], pose_run)], JOIN_TIMEOUT)
        got += WORKERS.run([create_and_run(nets[2], traj_run), lbs(body)], JOIN_TIMEOUT)
    _REAL_SYNC()
    for what, g, want in zip(('PoseNet 21', 'PoseNet 22', 'TrajNet', 'SMPL-X'), got, alone):
        diff = SM.differences(g, want)
        assert not diff, f'{what}: a handle created next to another one computes something else: {diff[:3]}'
    assert nets[0].native(dev).handle.value != nets[1].native(dev).handle.value


# ================================================================================================ coverage and numbers
def test_every_stream_taking_entry_point_was_called_on_two_streams_at_once_or_is_exempt():
    """Computed from the headers (stream_order.abi_stream_functions): every entry point with a stream parameter appears in the ledger
    of at least one pair on both of its streams, or stands in STREAM_PAIR_EXEMPT with its header sentence."""
    _alive()
    gated = {n: _gated(n) for n in GATED}
    threaded = {n: _threaded(n) for n in THREADED}
    on_two = set()
    for r in list(gated.values()) + list(threaded.values()):
        on_two |= {f for f, streams in r['streams'].items() if len(streams) >= 2}
    prose = SO.header_prose()
    assert set(STREAM_PAIR_EXEMPT) <= set(STREAM_AT) and all(s in prose for s in STREAM_PAIR_EXEMPT.values())
    missing = set(STREAM_AT) - on_two - set(STREAM_PAIR_EXEMPT)
    assert not missing, f'no pair calls {sorted(missing)} on two streams'
    from_threads = set().union(*(set(r['streams']) for r in threaded.values() if len(r['threads']) >= 2))
    assert set(RE.waiting_calls()) <= from_threads, sorted(set(RE.waiting_calls()) - from_threads)
    overlap = {n: r['overlap_ms'] for n, r in gated.items() if r['overlap_ms'] is not None}
    overlap3 = {n: r['overlap_ms'] for n, r in threaded.items() if r['overlap_ms'] is not None}
    handles = [n for n in overlap if n in G.HANDLES]
    numbers = dict(R=R, cases=len(ALL), gated_pairs=len(gated), threaded_pairs=len(threaded),
                   not_run=sorted(n for n in ALL if RE.not_together(n)), two_threads_only=sorted(n for n in RUN if n not in GATED),
                   thread_exempt=sorted(RE.THREAD_EXEMPT), entry_points=len(STREAM_AT), on_two_streams=len(on_two & set(STREAM_AT)),
                   logged_calls_gated=sum(r['calls'] for r in gated.values()), logged_calls_threaded=sum(r['calls'] for r in threaded.values()),
                   gate_ms=dict(min=1e3 * min(r['gate'] for r in gated.values()), max=1e3 * max(r['gate'] for r in gated.values()),
                                total=1e3 * sum(r['gate'] for r in gated.values())),
                   gates_still_closed_after_queueing=sum(bool(r['closed']) for r in gated.values()),
                   handle_pairs_overlap_ms=dict(min=min(overlap[n] for n in handles), max=max(overlap[n] for n in handles)),
                   pairs_that_overlapped=dict(gated=sum(v > 0 for v in overlap.values()), threaded=sum(v > 0 for v in overlap3.values())),
                   overlap_ms_gated={n: round(v, 3) for n, v in sorted(overlap.items())},
                   overlap_ms_threaded={n: round(v, 3) for n, v in sorted(overlap3.items())},
                   late_overlap_ms_gated_handles={n: round(gated[n]['late_overlap_ms'], 3) for n in sorted(handles)},
                   side_streams=dict(attempt=_harness()['attempt'], delay_units_per_ms=round(_harness()['rate'])))
    print('numbers:', json.dumps({k: v for k, v in numbers.items() if 'overlap_ms_' not in k}))
    path = os.environ.get('ROHM_REENTRANCY_JSON')
    if path:
        with open(path, 'w') as f:
            json.dump(numbers, f, indent=1, sort_keys=True)
