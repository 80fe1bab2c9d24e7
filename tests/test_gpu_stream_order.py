"""GPU: every entry point works on the caller's stream and, unless the header says so, never waits for it (include/rohm_hip.h,
"Conventions": "every launch goes on the caller-supplied hipStream_t; no hidden device synchronisation in forward / step / loop
calls").

tests/test_gpu_stale_memory.py poisons what a buffer holds and tests/test_gpu_bounds.py watches what lies around it; both run on
torch's default stream with their inputs long finished.  There a kernel, memset or copy that the library issues on stream 0 or on a
stream of its own without an event, or a wrapper that passes the wrong stream, is invisible: the stray work finds its inputs ready
and its consumer waits long enough anyway.  A hidden wait changes no result at all.  Here every case of that registry (imported, not
copied: `G.CASES`, `G._run`, `stale_memory.differences`, and `EXTRA` of tests/test_gpu_bounds.py) runs once more

  (1) plainly on the default stream: the baseline (`test_gpu_bounds._base`: two runs, so first-call probes are out of the way and
      repeatability is established; rule (b) of the stale-memory module applies unchanged, no case needs it), and a third plain run
      that records what the case uploads through `_d` and times every entry point's host side;
  (2) GATED (tests/stream_order.py): under `torch.cuda.stream(side)`, behind a delay kernel, with
        * every input that passes through `_d` (for the two training families every parameter's `.data` as well: the library reads
          the live parameters) in memory that was pre-filled before any gate -- floats NaN, integers and bools zero, a valid index --
          and receives its values by a device-to-device copy queued on the side stream behind the gate;
        * `stale_memory.poison(all-ones)`: the fills of outputs, workspaces, scratch and saved buffers run on the current stream, so
          behind the gate as well (the allocators arm a gate first if the last one may have run out);
        * the call log over the stream-taking functions of the loaded library: each call arms a further gate if less than
          `min_remaining` may be left, is held to `torch.cuda.current_stream()`, and notes whether the gate was STILL CLOSED when it
          returned.
  (3) The outputs equal the baseline BIT FOR BIT.  A stray launch runs at once, ahead of the gate: what it reads is not there yet, and
      what it writes is overwritten by the poison fill or the input copy that waits behind the gate.
  (4) Every logged call returned with the gate closed, or its function stands in `stream_order.SYNC_DOCUMENTED` with the header
      sentence that says it waits.  The cap outside that list is zero.  For the listed functions (3) still holds; only (4) is waived,
      and what such a call does AFTER its wait is not ordered by any gate.  rohm_trajnet_sample_loop is listed for its clip-resident
      form only: the `resident 0` cases must be, and are, wait-free.
  (5) Waits in Python (`.item()`, `.cpu()`, `torch.tensor(..., device=)`, torch.cuda.synchronize, the guided loop's poll) and in the
      `*_create` calls only drain a gate; the next allocation, input or entry point arms another.

The check can fail (run first; they pick the side stream): a three-step chain of torch ops whose middle step runs on
torch.cuda.default_stream(), or on a third stream without an event, comes out different from its plain run; a fake entry point that
synchronises the current stream is reported as unproven with its host time, one that only launches is proven; a stream argument
other than the current stream fails by name.  No library code is involved and no access leaves the test's own tensors.  With few
hardware queues two streams may share one, and work that shares the side stream's queue cannot overtake a gate: up to 8
torch.cuda.Stream() objects are tried and the module fails if none shows both strays.  On MI355X with 4 hardware queues the FIRST
stream showed both.  The same was checked once against the library itself, in an experiment copy with rohm_ddpm_step launching on
stream 0 and rohm_layernorm_f32 synchronising its stream: the ddpm case failed on (3)
(`ddpm_step`, element 0 NaN), the layernorm case on (4) (rohm_layernorm_f32, 25.0 ms: the whole gate), their neighbours passed.

Coverage: every function of the public headers with a `rohm_stream_t` parameter (78) returned at least once with the gate closed (75, among them
rohm_trajnet_sample_loop in its `resident 0` cases) or is documented as waiting (rohm_posenet_exchange_status, rohm_track_resample,
rohm_floor_hypotheses); STREAM_EXEMPT is empty.  The call log also holds stale_memory.COVERAGE and test_gpu_bounds.EXTRA_COVERAGE to
the truth: every family's cases really call what the tables claim (they did: no table needed a correction).

What stays unseen -- nobody should take it for covered:
  * a stray launch whose inputs were all ready before the gate and whose output nothing clobbers: in practice one that reads only
    weights or handle-owned tables and writes handle-owned memory;
  * inputs that bypass `_d` (listed in tests/test_gpu_bounds.py: index tensors made with torch.tensor(..., device=), what wrappers
    build from numpy arrays or host lists, tensors a case derives on the device, the weights of the inference handles); they are
    uploaded with a wait or computed in stream order, so they are simply ready;
  * anything after a documented wait inside the same call;
  * graph capture of the entry points: out of scope here, tests/test_gpu_graph_replay.py records and replays every one of them;
  * device tensors among the recorded inputs (the training parameters) are matched by shape and dtype, not by value.

Findings: nothing found.  Read before run, every launch, memset, copy, allocation and wait of rohm_amd/csrc: 147 kernel launch
sites; 124 take the stream they are handed -- the caller's, or `s2` for TrajControl's branch (below) -- and the 23 on stream 0 are all inside rohm_posenet_create,
rohm_trajnet_create, rohm_smplx_create, rohm_smplx_set_skinning and rohm_exchange_probe.  Outside those set-up calls: 15
hipMemsetAsync and 11 hipMemcpyAsync, all on the caller's stream; waits only where the header says so (rohm_profile_stop,
rohm_posenet_exchange_status, rohm_track_resample, rohm_floor_hypotheses, the clip-resident loop's one wait, the first-call probe of
rohm_gemm_res_layernorm_f32 / rohm_output_process_f32); one hipMalloc and one blocking hipMemcpy in the clip-resident loop, both
behind ROHM_TRAJ_RESIDENT_TIMELINE (a diagnostic print, after the documented wait).  TrajControl's control stream `s2` (trajnet.hip,
the launch-per-layer loop only; the single forward and the resident form do not use it): `s2` waits for an event recorded on the
caller's stream after the time table of each run of steps -- at step 0 that is after the cond encoders and the projected control
input, the only things the branch reads besides weights -- so it never reads a caller's tensor directly; the caller's stream waits
for the branch's event before mid_blk[1], the first consumer; `s2` waits for the "consumed" event of step i - 2 before it reuses a
set of residual buffers; an early return joins `s2` into the caller's stream.  The six TrajControl `resident 0` cases confirm it.
The loops' step table came from pageable host memory when this was read (hipMemcpyAsync, host to device, on the caller's stream:
one of the 11): the call returned with the gate closed and the results were bit-equal although the wrapper's array was gone by
then, i.e. eagerly the runtime stages it at the call.  Recorded into a graph it does not (tests/test_gpu_graph_replay.py), so the
timesteps travel in the kernel arguments since, and 10 hipMemcpyAsync are left.  No wrapper of rohm_amd/ passes anything but
torch's current stream.

Numbers (MI355X).  Gate length: the slowest host side of a single entry point in the plain runs is rohm_trajnet_train_backward,
1.54 ms (TrajControl; 1.33 ms TrajNet), then rohm_trajnet_sample_loop launch per layer 0.63 - 1.10 ms, rohm_trajnet_forward
0.22 - 0.44 ms, rohm_posenet_sample_loop 0.09 - 0.35 ms, rohm_posenet_train_backward 0.17 ms, rohm_posenet_forward 0.05 - 0.10 ms;
every other entry point stays below 0.025 ms.  4 x 1.54 ms = 6.2 ms is below the floor, so `min_remaining` is 10 ms for every case
(each case takes max(10 ms, 4 x its own slowest plain call)) and a gate is twice that, 20 ms, sized with a quarter more delay
cycles than calibrated (2.39e6 per ms).  A gate that is too short fails check (4); it cannot pass silently.
Sizes: 86 cases (81 of the registry, 5 of EXTRA), 190 logged calls and 318 gates in the gated runs, at most 11 gates per case;
the gated runs take 9.7 s in all, 0.025 - 0.41 s each (the three header cases: 3 / 2 / 4 calls, asserted from LOGGED_CALLS, one gate
and 0.026 s each).  Wall time of the whole module, 87 tests, run alone: 27 s as measured, next to the 21 s of
tests/test_gpu_bounds.py (the slowest test 1.5 s); after that module in one process the baselines are shared: 90 tests, 14.1 s
summed over its tests (the slowest 0.69 s)."""
import contextlib
import time

import pytest
import torch

import stale_memory as SM
import stream_order as SO
import test_gpu_bounds as B
import test_gpu_stale_memory as G
from helpers import seeded

pytestmark = pytest.mark.gpu
DEV = G.DEV
ALL = B.ALL                                     # the registry's cases and EXTRA of tests/test_gpu_bounds.py
STREAM_AT = SO.abi_stream_functions()           # entry point -> position of its stream argument
MIN_REMAINING = 0.010                           # seconds of gate a call must find left, at least (Numbers in the docstring)
MARGIN = 4                                      # ... and this many times the slowest call of the case's plain run
MAX_SIDE_STREAMS = 8
# the gated run of these cases logs exactly this many calls: two triangulations and the residuals; the fit with and without its
# optional operands; the four stream-taking functions of rohm_rig.h
LOGGED_CALLS = {'multiview[V4, N3, J22]': 3, 'fit_views[V3, N3, dead middle frame]': 2, 'rig[V4, N3, J22, Q6, K5]': 4}
assert set(LOGGED_CALLS) <= set(ALL)


# ================================================================================================ one measured run
@contextlib.contextmanager
def _patches(d, fam, arm=None):
    """The registry's `_d` replaced by `d`; for the training families every parameter's `.data` goes through it too (the library reads
    the live parameters); with `arm`, torch's uninitialised allocators call it first, so that stale_memory.poison -- entered later, by
    `G._run` -- fills behind a gate."""
    def parameters_through_d(make):
        def made(*a, **k):
            net = make(*a, **k)
            for _, q in net.named_parameters():
                q.data = G._d(q.data)
            return net
        return made

    def armed(real):
        def alloc(*a, **k):
            arm()
            return real(*a, **k)
        return alloc

    with pytest.MonkeyPatch.context() as m:
        m.setattr(G, '_d', d)
        if fam in B.PARAMS_ON_CANVASES:
            m.setattr(G, '_make_posenet', parameters_through_d(G._make_posenet))
            m.setattr(G, '_make_trajnet', parameters_through_d(G._make_trajnet))
        if arm is not None:
            m.setattr(torch, 'empty', armed(torch.empty))
            m.setattr(torch, 'empty_like', armed(torch.empty_like))
            m.setattr(torch.Tensor, 'new_empty', armed(torch.Tensor.new_empty))
        yield


def _measure(name, fn, fam, side, delay, rate, gated_fn=None, lib_obj=None, stream_at=None):
    """A plain run of `fn` on the default stream (inputs recorded, calls timed), then the gated run of `gated_fn or fn` on `side`:
    deferred inputs, all-ones poison, the call log.  -> dict(plain, got, error, log, plain_log, gates, min_remaining, inputs, seconds)"""
    from rohm_amd import _lib
    lib_obj = _lib.lib() if lib_obj is None else lib_obj
    stream_at = STREAM_AT if stream_at is None else stream_at
    inputs, plain_log = SO.DeferredInputs(DEV), SO.CallLog()
    with _patches(inputs.record, fam), plain_log.installed(lib_obj, stream_at):
        plain = G._run(fn, SM.ZEROS)
    slow, slow_fn = plain_log.slowest(skip={f for f in stream_at if SO.may_wait(f, name)})
    min_remaining = max(MIN_REMAINING, MARGIN * slow)
    with torch.cuda.stream(side):
        inputs.stage()
    torch.cuda.synchronize()                    # the pre-fills are written before any gate is armed
    gates = SO.Gates(side, 2.0 * min_remaining, delay, rate)
    log = SO.CallLog(gates, min_remaining)
    arm = lambda: gates.ensure_gate(min_remaining)
    got, error, t0 = None, None, time.perf_counter()
    try:
        with torch.cuda.stream(side), _patches(lambda t: inputs.replay(t, arm), fam, arm), log.installed(lib_obj, stream_at):
            gates.arm()
            got = G._run(gated_fn or fn, SO.ONES)
    except Exception as e:                      # kept for the case's own test; the coverage test goes on
        error = e
    finally:
        torch.cuda.synchronize()
    return dict(plain=plain, got=got, error=error, log=log, plain_log=plain_log, gates=gates.count, min_remaining=min_remaining,
                slowest=(slow, slow_fn), inputs=inputs, seconds=time.perf_counter() - t0)


# ================================================================================================ the check can fail: planted strays
def _chain(wrong=None):
    """Three torch ops on the test's own tensors; the middle one runs on the stream `wrong()` returns (None: on the current one)."""
    a = G._d(seeded(1, 4096))
    b = torch.empty_like(a)
    torch.mul(a, 2.0, out=b)
    c = torch.empty_like(a)
    with torch.cuda.stream(wrong()) if wrong is not None else contextlib.nullcontext():
        torch.add(b, 1.0, out=c)
    d = torch.empty_like(a)
    torch.mul(c, 3.0, out=d)
    return [('d', d)]


_HARNESS = {}


def _harness():
    """The side stream, picked by the two planted strays: with few hardware queues two streams may share one, and work that shares the
    side stream's queue cannot overtake a gate.  -> dict(side, attempt, delay, rate, tried)"""
    if not _HARNESS:
        delay, guess = SO.torch_delay()
        third = torch.cuda.Stream()
        strays = {'default stream': torch.cuda.default_stream, 'third stream, no event': lambda: third}
        tried, keep = [], []
        _HARNESS.update(side=None, attempt=None, delay=delay, rate=None, tried=tried, third=third)
        for attempt in range(1, MAX_SIDE_STREAMS + 1):
            side = torch.cuda.Stream()
            keep.append(side)
            rate = 1.25 * SO.calibrate(delay, guess, side)      # (a quarter more: a gate may be longer than asked for, never shorter)
            seen = {}
            for kind, wrong in strays.items():
                r = _measure('planted stray: ' + kind, _chain, 'planted', side, delay, rate, gated_fn=lambda w=wrong: _chain(w))
                assert r['error'] is None, r['error']
                seen[kind] = bool(SM.differences(r['got'], r['plain']))
            tried.append(seen)
            if all(seen.values()):
                _HARNESS.update(side=side, attempt=attempt, rate=rate)
                break
    assert _HARNESS['side'] is not None, (f'none of {MAX_SIDE_STREAMS} streams shows both planted strays: {_HARNESS["tried"]}; the rest '
                                          f'of the module would prove nothing')
    return _HARNESS


def test_both_planted_strays_are_reported_and_pick_the_side_stream():
    """A three-step chain of torch ops whose middle step runs on torch's default stream / on a third stream without an event must
    come out different from the plain run.  No library code runs and no access leaves the test's own tensors."""
    h = _harness()
    print(f'side stream: attempt {h["attempt"]} of {MAX_SIDE_STREAMS}, {h["rate"]:.0f} delay units per ms, tried {h["tried"]}')
    assert all(h['tried'][-1].values()) and h['attempt'] == len(h['tried'])
    r = _measure('planted: no stray', _chain, 'planted', h['side'], h['delay'], h['rate'])      # ... and the chain in stream order passes
    assert r['error'] is None and not SM.differences(r['got'], r['plain']) and r['inputs'].complete() and r['gates'] >= 1


class _StandIn:
    """Two fake entry points made of torch ops: one queues work on the current stream, one waits for it."""

    def rohm_fake_launch(self, x, stream):
        x.mul_(2.0)
        return 0

    def rohm_fake_wait(self, x, stream):
        x.add_(1.0)
        torch.cuda.current_stream().synchronize()
        return 0


def test_a_planted_wait_is_reported():
    from rohm_amd._lib import stream_ptr
    h, fake = _harness(), _StandIn()

    def fn():
        x = G._d(seeded(2, 4096))
        fake.rohm_fake_launch(x, stream_ptr())
        fake.rohm_fake_wait(x, stream_ptr())
        fake.rohm_fake_launch(x, stream_ptr())
        return [('x', x)]
    r = _measure('planted wait', fn, 'planted', h['side'], h['delay'], h['rate'], lib_obj=fake,
                 stream_at={'rohm_fake_launch': 1, 'rohm_fake_wait': 1})
    assert r['error'] is None and not SM.differences(r['got'], r['plain'])
    assert [(f, closed) for f, _, closed in r['log'].calls] == [('rohm_fake_launch', True), ('rohm_fake_wait', False), ('rohm_fake_launch', True)]
    unproven = r['log'].unproven()
    assert [f for f, _ in unproven] == ['rohm_fake_wait'] and unproven[0][1] > 0.0
    assert r['gates'] >= 2                      # the wait drained the first gate; the next call armed another
    assert fake.rohm_fake_wait.__func__ is _StandIn.rohm_fake_wait          # the originals are back


def test_a_wrong_stream_argument_fails_by_name():
    h, fake = _harness(), _StandIn()
    r = _measure('planted wrong stream', lambda: [('x', G._d(seeded(3, 16)))], 'planted', h['side'], h['delay'], h['rate'], lib_obj=fake,
                 stream_at={'rohm_fake_launch': 1},
                 gated_fn=lambda: [('x', G._d(seeded(3, 16)))] + [('rc', torch.tensor(fake.rohm_fake_launch(torch.ones(4, device=DEV), None)))])
    assert isinstance(r['error'], AssertionError) and 'rohm_fake_launch was handed the stream 0x0' in str(r['error'])


# ================================================================================================ every case
_RESULTS = {}


def _result(name):
    """The case's gated run held against its plain runs, computed once: dict(diff, unproven, calls, proven, error, ...)."""
    if name not in _RESULTS:
        h = _harness()
        base, repeatable = B._base(name)        # two plain runs on the default stream (first-call probes out of the way; rule (b))
        r = _measure(name, ALL[name], G.family(name), h['side'], h['delay'], h['rate'])
        out = dict(error=r['error'], diff=None, oracle_error=None, repeatable=repeatable, gates=r['gates'], seconds=r['seconds'],
                   min_remaining=r['min_remaining'], slowest=r['slowest'], calls=r['log'].functions() | r['plain_log'].functions(),
                   proven=r['log'].proven(), unproven=r['log'].unproven(lambda f: SO.may_wait(f, name)),
                   n_calls=len(r['log'].calls), plain_diff=SM.differences(r['plain'], base) if repeatable else [],
                   inputs=(r['inputs'].replayed, len(r['inputs'].staged)))
        if r['error'] is None:
            if repeatable:
                out['diff'] = SM.differences(r['got'], base)
            else:
                try:
                    G.ORACLE[name](r['got'])
                except AssertionError as e:
                    out['oracle_error'] = e
        _RESULTS[name] = out
    return _RESULTS[name]


@pytest.mark.parametrize('name', sorted(ALL))
def test_calls_work_on_the_callers_stream_and_do_not_wait(name):
    r = _result(name)
    slow, slow_fn = r['slowest']
    print(f'{name}: {r["n_calls"]} logged calls, {r["gates"]} gates of {2e3 * r["min_remaining"]:.1f} ms, gated run {r["seconds"]:.3f} s, '
          f'slowest plain call {slow_fn} {1e3 * slow:.3f} ms, inputs {r["inputs"]}')
    if r['error'] is not None:
        raise r['error']
    assert not r['plain_diff'], f'{name}: recording the inputs changes the plain run: {r["plain_diff"][:3]}'
    assert r['inputs'][0] == r['inputs'][1], f'{name}: the gated run asked for {r["inputs"][0]} of the plain run\'s {r["inputs"][1]} inputs'
    if r['oracle_error'] is not None:
        raise r['oracle_error']
    assert not r['diff'], (f'{name}: the result changes when the caller\'s stream is held back and the inputs arrive on it: '
                           f'{r["diff"][:3]} (output, (first differing element, value here, baseline))')
    assert not r['unproven'], (f'{name}: calls returned with the gate open (they waited for the stream, or took longer than '
                               f'{1e3 * r["min_remaining"]:.1f} ms): {[(f, f"{1e3 * s:.3f} ms") for f, s in r["unproven"]]}')
    assert r['n_calls'] > 0 and r['gates'] <= 64, (r['n_calls'], r['gates'])
    assert r['n_calls'] == LOGGED_CALLS.get(name, r['n_calls']), r['n_calls']


def test_every_stream_taking_entry_point_is_proven_documented_or_exempt_and_the_coverage_tables_are_true():
    """Over all cases: every header function with a stream parameter returned at least once with the gate still closed, or stands in
    SYNC_DOCUMENTED / STREAM_EXEMPT; and every family's cases really called what stale_memory.COVERAGE / EXTRA_COVERAGE claim."""
    results = {name: _result(name) for name in sorted(ALL)}
    proven = set().union(*(r['proven'] for r in results.values()))
    missing = set(STREAM_AT) - proven - set(SO.SYNC_DOCUMENTED) - set(SO.STREAM_EXEMPT)
    assert not missing, f'no case proves {sorted(missing)} wait-free'
    # the loop that is documented as waiting in one form only is proven in the other
    assert 'rohm_trajnet_sample_loop' in set().union(*(r['proven'] for n, r in results.items() if 'resident 0' in n))
    called = {}
    for name, r in results.items():
        called.setdefault(G.family(name), set()).update(r['calls'])
    claims = dict(SM.COVERAGE)
    claims.update(B.EXTRA_COVERAGE)
    wrong = {fam: sorted(set(fs) & set(STREAM_AT) - called.get(fam, set())) for fam, fs in claims.items()}
    wrong = {fam: fs for fam, fs in wrong.items() if fs}
    assert not wrong, f'coverage tables name entry points their family\'s cases never call: {wrong}'
    times = sorted(((r['slowest'][0], r['slowest'][1], n) for n, r in results.items()), reverse=True)[:5]
    print('slowest plain calls:', [(f'{1e3 * s:.3f} ms', f, n) for s, f, n in times])
    print('gates:', sum(r['gates'] for r in results.values()), 'calls:', sum(r['n_calls'] for r in results.values()),
          'max min_remaining (ms):', 1e3 * max(r['min_remaining'] for r in results.values()),
          'gated seconds:', sum(r['seconds'] for r in results.values()))
    print('proven:', len(proven & set(STREAM_AT)), 'of', len(STREAM_AT), '; documented as waiting:', sorted(set(STREAM_AT) & set(SO.SYNC_DOCUMENTED)))
