"""TEST INFRASTRUCTURE ONLY (host side of tests/test_gpu_stream_order.py): a gate that holds one stream back, a call log over the
loaded library, inputs whose values arrive behind the gate, the parser that lists every entry point of the public headers with a
`rohm_stream_t` parameter, and the two lists that say which of them may wait (SYNC_DOCUMENTED) or are not run (STREAM_EXEMPT).
Nothing in rohm_amd/ imports this module.

include/rohm_hip.h ("Conventions") promises that every launch goes on the caller's stream and that no forward / step / loop call
waits for the device.  On torch's default stream, with inputs long finished, neither a launch on another stream nor a hidden wait
changes a result.  Here the caller's stream is a side stream that a GATE (a delay kernel) holds back while the host runs ahead:

  * `Gates`: the delay is torch.cuda._sleep (or, without it, a chain of matmuls), calibrated once with events; an event recorded
    behind every gate tells whether it is still closed.  A gate cannot start before the host armed it, so host time since arming is
    an upper bound on how much of it has run; `ensure_gate(min_remaining)` arms a further one when less may be left.
  * `CallLog`: for the duration of a test the stream-taking `rohm_*` attributes of the cached CDLL are recording wrappers: arm a gate
    if need be, hold the stream argument to torch's current stream (a wrapper that hands the library another stream fails there, by
    name), call through, note (function, host seconds, gate still closed at return).  A call that returns with the gate closed has
    not waited for the stream.
  * `DeferredInputs`: what a case uploads through its `_d` is recorded in a plain run and staged on the device; in the gated run `_d`
    returns memory pre-filled BEFORE any gate (floats: all-ones bytes, NaN; integers and bools: zeros, a valid index, so a stray
    kernel computes something wrong and does not address outside a buffer) into which the values are copied device-to-device on the
    side stream, behind the gate, without blocking the host.  The gated run must ask for the same sequence of inputs.

A launch on any other stream runs at once, ahead of the gate: what it reads is not there yet, and what it writes is overwritten by
the poison fill of the allocation (stale_memory.poison, on the current stream) or by the input copy that waits behind the gate."""
import contextlib
import ctypes as C
import re
import time

import torch

import stale_memory as SM

ONES = SM.PATTERNS['ones']


# ---- the ABI's stream parameters ---------------------------------------------------------------------------------------------
def abi_stream_functions(text=None):
    """{entry point: position of its `rohm_stream_t` parameter} for every declaration of the public headers that has one (next to
    stale_memory.abi_buffer_functions / abi_pointer_functions).  A declaration with two stream parameters is refused: the call log
    could not tell which one is the caller's."""
    out = {}
    for name, params in SM.declarations(text):
        at = [i for i, param in enumerate(params) if re.match(r'^\s*(?:const\s+)?rohm_stream_t\s+\w+\s*$', param)]
        if len(at) > 1:
            raise ValueError(f'{name} has {len(at)} rohm_stream_t parameters')
        if at:
            out[name] = at[0]
    return out


def header_prose(text=None):
    """The public headers as one line of text: comment decoration (` * ` at the start of a line) and line breaks become single spaces, so a
    sentence that the header wraps can be looked up as written."""
    text = re.sub(r'\n\s*\*(?!/)', ' ', SM.abi_text() if text is None else text)
    return re.sub(r'\s+', ' ', text)


# entry point -> the header sentence that says it waits (built by reading the header, not by running).  For these the bit-equality
# check of tests/test_gpu_stream_order.py still holds; only "the gate is still closed at return" is waived, and what such a call does
# AFTER its wait is not ordered by any gate.  Functions without a stream parameter are listed for the record (the call log does not
# see them; a gate they drain is armed again by the next logged call).
_SETUP = ('Set-up calls say so where they synchronise: *_create, rohm_exchange_probe, rohm_posenet_set_exchange(h, 1), the status read '
          'rohm_posenet_exchange_status')
SYNC_DOCUMENTED = {
    'rohm_posenet_create': _SETUP,
    'rohm_trajnet_create': _SETUP,
    'rohm_smplx_create': _SETUP,
    'rohm_exchange_probe': 'Allocates, launches on the null stream and synchronises the device: a set-up call.',
    'rohm_posenet_set_exchange': 'that re-probe synchronises the device, so on = 1 is a control call between runs.',
    'rohm_posenet_exchange_status': 'This call synchronises `stream`, returns ROHM_ERR_EXCHANGE (and clears the word) if it is set',
    'rohm_trajnet_sample_loop': "when it runs, rohm_trajnet_sample_loop waits for the stream once at its end to read the exchange's error word",
    'rohm_track_resample': 'the ascending indices of the source frames that have a fit (read back and checked here: one stream '
                           'synchronisation per call)',
    'rohm_floor_hypotheses': 'triples [K,3] int32 indices into points (read back and checked here: one stream synchronisation per call',
    'rohm_profile_stop': 'rohm_profile_stop synchronises the recorded events and aggregates per kernel label',
}
# entry point -> when its sentence applies, as a predicate on the case's name; everywhere else the call must be wait-free
SYNC_ONLY_IN = {
    'rohm_trajnet_sample_loop': lambda case: 'resident 1' in case,      # the clip-resident form; ROHM_TRAJ_RESIDENT=0 keeps it wait-free
}

# stream-taking entry points that no case of the registry runs, each with its reason (follows stale_memory.EXEMPT)
STREAM_EXEMPT = {}      # (none today: a new entry needs a sentence in the pull request that adds it saying why no case can run it)


def may_wait(function, case):
    """Whether `function`, called by the case named `case`, is documented as waiting."""
    return function in SYNC_DOCUMENTED and SYNC_ONLY_IN.get(function, lambda _: True)(case)


# ---- the gate ----------------------------------------------------------------------------------------------------------------
def torch_delay():
    """(delay(units): queue a delay of `units` on the current stream, a first guess of units per millisecond).  torch.cuda._sleep
    counts device clock cycles; without it a chain of 1024 x 1024 matmuls stands in (one unit each)."""
    if hasattr(torch.cuda, '_sleep'):
        return (lambda units: torch.cuda._sleep(int(units))), 1.0e5
    a = torch.full((1024, 1024), 1.0 / 1024, device='cuda')
    b = torch.empty_like(a)

    def chain(units):
        for _ in range(int(units)):
            torch.mm(a, a, out=b)
    return chain, 20.0


def calibrate(delay, guess, stream, target_ms=4.0, rounds=3):
    """Units of `delay` per millisecond on `stream`, measured with events: the LARGEST of `rounds` measurements of a delay of about
    `target_ms`, so that a gate sized with it is not shorter than asked for while the clock ramps."""
    def measure(units):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        delay(units)
        b.record(stream)
        b.synchronize()
        return max(a.elapsed_time(b), 1e-3)
    with torch.cuda.stream(stream):
        units = max(1.0, guess * 0.5)
        rate = units / measure(units)                   # (launch overhead included: an under-estimate, refined below)
        for _ in range(2):
            units = max(1.0, rate * target_ms)
            rate = units / measure(units)
        measure(max(1.0, rate * 5.0 * target_ms))       # keep the device busy for a while first: its clock has ramped by the time of
        units = max(1.0, rate * target_ms)              # the measurements that count
        return max(units / measure(units) for _ in range(rounds))


class Gates:
    """Delays queued on `stream`, each `length` seconds long, with an event recorded behind each.  `arm` notes the host clock BEFORE
    it queues the delay: the delay cannot have started earlier, so it ends no earlier than that time + length."""

    def __init__(self, stream, length, delay, units_per_ms, event=None, clock=time.perf_counter, on_stream=None):
        self.stream, self.length, self.delay, self.units_per_ms = stream, float(length), delay, units_per_ms
        self.event_factory = event or (lambda: torch.cuda.Event())
        self.on_stream = on_stream or torch.cuda.stream         # (the delay goes on `stream` whatever the current stream is)
        self.clock = clock
        self.armed_at, self.event, self.count = None, None, 0

    def arm(self):
        t = self.clock()
        with self.on_stream(self.stream):
            self.delay(self.units_per_ms * self.length * 1e3)
            ev = self.event_factory()
            ev.record(self.stream)
        self.armed_at, self.event = t, ev
        self.count += 1

    def may_remain(self):
        """A lower bound, by the host clock, on what is left of the last gate (seconds; <= 0: it may be open)."""
        return -1.0 if self.event is None else self.armed_at + self.length - self.clock()

    def ensure_gate(self, min_remaining):
        if not min_remaining < self.length:
            raise ValueError(f'a gate of {self.length} s can never have {min_remaining} s left')
        if self.may_remain() < min_remaining:
            self.arm()

    def closed(self):
        """Whether the last gate is still closed, as the device says (its event has not completed)."""
        return self.event is not None and not self.event.query()


# ---- the call log ------------------------------------------------------------------------------------------------------------
def stream_value(arg):
    """The address in a stream argument as ctypes takes it: a c_void_p, an int or None (the null stream)."""
    if isinstance(arg, C.c_void_p):
        arg = arg.value
    return int(arg or 0)


def current_stream_value():
    return int(torch.cuda.current_stream().cuda_stream)


class CallLog:
    """Recording wrappers over the stream-taking functions of a library object.  `calls` holds (function, host seconds, gate still
    closed at return -- None without gates).  With `gates`, every call first makes sure `min_remaining` seconds of gate are left."""

    def __init__(self, gates=None, min_remaining=0.0, current_stream=current_stream_value, clock=time.perf_counter):
        self.gates, self.min_remaining, self.current_stream, self.clock = gates, min_remaining, current_stream, clock
        self.calls = []

    def _wrap(self, name, real, at):
        def logged(*args):
            if self.gates is not None:
                self.gates.ensure_gate(self.min_remaining)
            got, want = stream_value(args[at]), self.current_stream()
            assert got == want, f'{name} was handed the stream {got:#x}, the current stream is {want:#x}'
            t0 = self.clock()
            rc = real(*args)
            seconds = self.clock() - t0
            self.calls.append((name, seconds, self.gates.closed() if self.gates is not None else None))
            return rc
        logged.__wrapped__ = real
        return logged

    @contextlib.contextmanager
    def installed(self, obj, stream_at):
        """Replace `obj.<name>` for every name of `stream_at` ({name: position of the stream argument}); the originals are put back
        on exit, whatever happened."""
        originals = {}
        try:
            for name, at in stream_at.items():
                originals[name] = getattr(obj, name)
                setattr(obj, name, self._wrap(name, originals[name], at))
            yield self
        finally:
            for name, real in originals.items():
                setattr(obj, name, real)

    def functions(self):
        return {name for name, _, _ in self.calls}

    def slowest(self, skip=()):
        """(seconds, function) of the slowest logged call of a function not in `skip`, or (0.0, None)."""
        return max(((s, name) for name, s, _ in self.calls if name not in skip), default=(0.0, None))

    def unproven(self, may_wait=lambda name: False):
        """[(function, host seconds)] of the calls that returned with the gate open and are not allowed to wait."""
        return [(name, s) for name, s, closed in self.calls if closed is False and not may_wait(name)]

    def proven(self):
        return {name for name, _, closed in self.calls if closed}


# ---- deferred inputs ---------------------------------------------------------------------------------------------------------
def prefill_word(dtype):
    """All-ones bytes (NaN) for floating types, zeros (a valid index) for integers and bools."""
    return ONES if (dtype.is_floating_point or dtype.is_complex) else SM.ZEROS


class DeferredInputs:
    """record (plain run) -> stage (before any gate) -> replay (gated run).

    `record(t)` stands in for a case's `_d` in a plain run: it notes `t` and returns `t` on the device.  `stage()` puts every noted
    tensor on the device and allocates its pre-filled destination; the caller synchronises after it.  `replay(t)` stands in for `_d`
    in the gated run: the i-th call must ask for what the i-th `record` was given (shape, dtype and, for host tensors, every bit),
    queues the device-to-device copy on the current stream and returns the destination.  Tensors that already live on the device (a
    training family's parameters) are noted as clones and compared by shape and dtype only: comparing their values would wait."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.recorded, self.staged = [], []
        self.replayed = 0

    def record(self, t):
        assert t.is_contiguous(), f'input #{len(self.recorded)} {tuple(t.shape)} is not contiguous'
        on_host = t.device.type == 'cpu' and self.device.type != 'cpu'
        self.recorded.append(t.detach() if on_host else t.detach().clone())
        return t.to(self.device)

    def stage(self):
        assert not self.staged
        for t in self.recorded:
            src = t.to(self.device)
            dst = SM.fill_bytes(SM._REAL_EMPTY(src.shape, dtype=src.dtype, device=self.device), prefill_word(src.dtype))
            self.staged.append((src, dst))
        return self

    def replay(self, t, before_copy=None):
        i = self.replayed
        assert i < len(self.staged), f'the gated run asks for input #{i}, the plain run asked for {len(self.staged)}'
        want = self.recorded[i]
        assert tuple(t.shape) == tuple(want.shape) and t.dtype == want.dtype, \
            f'input #{i}: the gated run asks for {tuple(t.shape)} {t.dtype}, the plain run asked for {tuple(want.shape)} {want.dtype}'
        if t.device.type == 'cpu':
            assert SM.first_difference(t.detach(), want.cpu()) is None, f'input #{i} differs from the plain run'
        src, dst = self.staged[i]
        if before_copy is not None:
            before_copy()
        dst.copy_(src, non_blocking=True)
        self.replayed += 1
        return dst

    def complete(self):
        return self.replayed == len(self.staged)
