"""TEST INFRASTRUCTURE ONLY (host side of tests/test_gpu_reentrancy.py): a ledger of who was handed which memory, the rule that says
which two calls of it are unordered, the device-interval overlap of two sides, two long-lived worker threads released by a barrier, and
the tables of pairs that are not run together.  Nothing in rohm_amd/ imports this module.

include/rohm_hip.h ("Conventions") promises that calls are re-entrant across streams given distinct workspaces.  Whether two callers
WERE given distinct memory is a question about arguments, not about timing:

  * `abi_operands`: for every entry point of the public headers with a `rohm_stream_t` parameter (stream_order.abi_stream_functions)
    the positions of its stream, its handle (`rohm_*_t*`), its sized buffers (`void* ws, size_t ws_bytes`:
    stale_memory.abi_buffer_functions) and its other pointers to numbers (stale_memory.abi_pointer_functions), each classed by the
    header's own `const` as read or written.  Tables of pointers (`float* const*`) are host arrays and carry no range.
  * `Ledger`: recording wrappers over those functions of a library object, as stream_order.CallLog (whose stream check it repeats).
    Every call notes its thread, stream, handle and the address range of every non-NULL operand: [ptr, ptr + bytes) for a sized
    buffer, the extent of the tensor for a pointer that a wrapper took with Tensor.data_ptr() while the ledger was installed (the
    ledger wraps that method on the class for as long as it is installed; device tensors only).  A pointer of unknown provenance
    (a host array, a host scalar) carries no range: host memory is the calling thread's own.  The ledger also notes the host waits it
    can see (torch.cuda.synchronize, Stream.synchronize; or, `synchronize='skip'`, turns torch.cuda.synchronize into nothing for a
    run whose calls are queued behind a closed gate) and can DEFER named calls (the status read that waits) until the gate is open.
  * `conflicts`: two calls on different streams are ORDERED only if the first one returned before a host wait that covers its stream
    began and that wait ended before the second call was entered -- a device or stream synchronisation, or a call the header documents
    as waiting for its stream (it drains what was queued before it; what it queues itself after its wait is ordered by nothing).
    Between two unordered calls no written range of one may intersect a written or read range of the other.  Ranges that merely touch
    do not intersect.  What the ledger cannot see (a `.item()`, a blocking copy) orders nothing: the check errs towards reporting.
  * `overlap_ms`: the intersection of two device intervals from four events, through `elapsed_time` across the streams.
  * `Workers`: two threads that live as long as the module (the library keeps a control stream per host thread: fresh threads per
    test would leave one behind each), released together by a threading.Barrier, joined with a timeout; after a timeout the object
    refuses every further job."""
import contextlib
import ctypes as C
import itertools
import queue
import re
import threading

import torch

import stale_memory as SM
import stream_order as SO

R = 8                       # calls queued per side


# ---- the ABI's operands --------------------------------------------------------------------------------------------------------
_POINTER = re.compile(r'^\s*(const\s+)?' + SM._POINTEE + r'\s*(?:const\s*)?\*\s*(const\s*\*\s*)?(?:const\s+)?(\w+)\s*$')
_HANDLE = re.compile(r'^\s*(?:const\s+)?rohm_\w+_t\s*\*\s*(\w+)\s*$')


def abi_operands(text=None):
    """{entry point: dict(stream, handle (or None), operands [(name, position, position of its byte count or None, written)])} for
    every declaration with a `rohm_stream_t` parameter."""
    stream_at, sized = SO.abi_stream_functions(text), SM.abi_buffer_functions(text)
    out = {}
    for name, params in SM.declarations(text):
        if name not in stream_at:
            continue
        handle = next((i for i, p in enumerate(params) if _HANDLE.match(p)), None)
        operands = []
        for i, p in enumerate(params):
            m = _POINTER.match(p)
            if m is None or m.group(2):                         # (a table of pointers is a host array)
                continue
            bytes_at = i + 1 if m.group(3) in sized.get(name, ()) else None
            operands.append((m.group(3), i, bytes_at, m.group(1) is None))
        out[name] = dict(stream=stream_at[name], handle=handle, operands=operands)
    return out


def address(arg):
    """The address in a pointer argument as ctypes takes it: None, an int, a c_void_p, a typed pointer, byref(x); 0 if it has none."""
    if arg is None:
        return 0
    if isinstance(arg, int):
        return arg
    if isinstance(arg, C.c_void_p):
        return int(arg.value or 0)
    if isinstance(arg, C._Pointer):
        return int(C.cast(arg, C.c_void_p).value or 0)
    obj = getattr(arg, '_obj', None)                             # byref(x)
    return C.addressof(obj) if obj is not None else 0


def extent_bytes(t):
    """Bytes from the first to the last element of a tensor, whatever its strides."""
    if t.numel() == 0:
        return 0
    return (sum((n - 1) * abs(s) for n, s in zip(t.shape, t.stride())) + 1) * t.element_size()


# ---- the ledger ----------------------------------------------------------------------------------------------------------------
class Ledger:
    """`entries`: dicts in the order the calls RETURNED.  kind 'call': function, thread, stream, handle, writes / reads
    [(operand, lo, hi)], enter / leave (ticks of one counter), rc, waits (the header documents the call as waiting and `waits(name)`
    says the sentence applies here), deferred.  kind 'sync': stream (None: the device), enter, leave."""

    def __init__(self, operands=None, waits=lambda name: False, defer=(), current_stream=SO.current_stream_value, synchronize='note'):
        assert synchronize in ('note', 'skip', None)
        self.operands = abi_operands() if operands is None else operands
        self.waits, self.defer, self.current_stream, self.synchronize = waits, frozenset(defer), current_stream, synchronize
        self.entries, self.deferred, self.sizes = [], [], {}
        self._ticks, self._lock = itertools.count(1), threading.Lock()

    def tick(self):
        with self._lock:
            return next(self._ticks)

    def _ranges(self, op, args):
        writes, reads = [], []
        for name, at, bytes_at, written in op['operands']:
            lo = address(args[at])
            if not lo:
                continue                                         # NULL: an optional operand that is not there
            n = int(getattr(args[bytes_at], 'value', args[bytes_at])) if bytes_at is not None else self.sizes.get(lo)
            if n:
                (writes if written else reads).append((name, lo, lo + n))
        return writes, reads

    def _wrap(self, name, real, op):
        def logged(*args):
            enter = self.tick()
            got, want = SO.stream_value(args[op['stream']]), self.current_stream()
            assert got == want, f'{name} was handed the stream {got:#x}, the current stream is {want:#x}'
            writes, reads = self._ranges(op, args)
            entry = dict(kind='call', function=name, thread=threading.get_ident(), stream=got, writes=writes, reads=reads, enter=enter,
                         handle=address(args[op['handle']]) if op['handle'] is not None else None, deferred=name in self.defer,
                         waits=name not in self.defer and bool(self.waits(name)))
            if entry['deferred']:
                self.deferred.append((name, real, args))
                rc = 0
            else:
                rc = real(*args)
            entry.update(rc=rc, leave=self.tick())
            self.entries.append(entry)
            return rc
        logged.__wrapped__ = real
        return logged

    def note_sync(self, stream, wait):
        enter = self.tick()
        wait()
        self.entries.append(dict(kind='sync', stream=stream, enter=enter, leave=self.tick()))

    def run_deferred(self):
        """Make the deferred calls now (the caller has opened the gate) -> [(function, return code)]."""
        done, self.deferred = [(name, real(*args)) for name, real, args in self.deferred], []
        return done

    @contextlib.contextmanager
    def installed(self, obj, patch_torch=True):
        """Wrap `obj.<name>` for every entry point of `operands`, Tensor.data_ptr, and the host waits; everything is put back on exit,
        whatever happened.  Install before worker threads start and leave after they are joined."""
        import pytest
        with pytest.MonkeyPatch.context() as m:
            for name, op in self.operands.items():
                m.setattr(obj, name, self._wrap(name, getattr(obj, name), op))
            if patch_torch:
                real_ptr = torch.Tensor.data_ptr

                def data_ptr(t):
                    p = real_ptr(t)
                    if p and t.is_cuda:
                        self.sizes[p] = extent_bytes(t)
                    return p
                m.setattr(torch.Tensor, 'data_ptr', data_ptr)
                if self.synchronize == 'skip':
                    m.setattr(torch.cuda, 'synchronize', lambda device=None: None)
                elif self.synchronize == 'note':
                    real_sync, real_stream_sync = torch.cuda.synchronize, torch.cuda.Stream.synchronize
                    m.setattr(torch.cuda, 'synchronize', lambda device=None: self.note_sync(None, lambda: real_sync(device)))
                    m.setattr(torch.cuda.Stream, 'synchronize', lambda s: self.note_sync(int(s.cuda_stream), lambda: real_stream_sync(s)))
            yield self

    def calls(self):
        return [e for e in self.entries if e['kind'] == 'call']

    def streams_of(self):
        """{function: the streams it was called on}"""
        out = {}
        for e in self.calls():
            out.setdefault(e['function'], set()).add(e['stream'])
        return out


def ordered(first, second, entries):
    """Whether everything `first` queued is complete, as the host can tell, before `second` was entered."""
    if first['leave'] >= second['enter']:
        return False
    for e in entries:
        if e['enter'] > first['leave'] and e['leave'] < second['enter']:
            if e['kind'] == 'sync' and e['stream'] in (None, first['stream']):
                return True
            if e['kind'] == 'call' and e['waits'] and e['stream'] == first['stream']:
                return True
    return False


def conflicts(entries, host_order=True):
    """[(call a, call b, operand of a, operand of b, lo, hi)]: the ranges that two unordered calls on different streams share, at least
    one side writing.  `host_order=False` takes no wait for an ordering: whatever two streams were handed in one run is held to be
    distinct (for the cases that wait inside and run from two threads only, where an ordering is an accident of timing)."""
    calls = [e for e in entries if e['kind'] == 'call']
    out = []
    for i, a in enumerate(calls):
        for b in calls[i + 1:]:
            if a['stream'] == b['stream']:
                continue
            if host_order and (ordered(a, b, entries) or ordered(b, a, entries)):
                continue
            for x, y in ((a, b), (b, a)):
                for wn, wlo, whi in x['writes']:
                    for on, olo, ohi in (y['writes'] if x is a else []) + y['reads']:      # (write / write is reported once)
                        if wlo < ohi and olo < whi:
                            out.append((x, y, wn, on, max(wlo, olo), min(whi, ohi)))
    return out


def describe(conflict):
    x, y, wn, on, lo, hi = conflict
    kind = 'writes' if any(n == on and l < hi and lo < h for n, l, h in y['writes']) else 'reads'
    return (f'{x["function"]} on stream {x["stream"]:#x} (thread {x["thread"]}) writes `{wn}` and {y["function"]} on stream '
            f'{y["stream"]:#x} (thread {y["thread"]}) {kind} `{on}`: shared range [{lo:#x}, {hi:#x}), {hi - lo} bytes, no host-visible '
            f'ordering between the two calls')


def report(entries, limit=3, host_order=True):
    found = conflicts(entries, host_order)
    return [describe(c) for c in found[:limit]] + ([f'... and {len(found) - limit} more'] if len(found) > limit else [])


# ---- device intervals ------------------------------------------------------------------------------------------------------------
def overlap_ms(a, b, elapsed=lambda x, y: x.elapsed_time(y)):
    """The intersection of the device intervals a = (first, last) and b = (first, last), in milliseconds (<= 0: they do not
    intersect), measured from a's first event."""
    a1, b0, b1 = elapsed(a[0], a[1]), elapsed(a[0], b[0]), elapsed(a[0], b[1])
    return min(a1, b1) - max(0.0, b0)


# ---- two host threads ------------------------------------------------------------------------------------------------------------
class WorkerTimeout(AssertionError):
    pass


class Workers:
    """`n` threads, started at the first job and kept.  `run(jobs, timeout)`: job i runs on thread i after all have met at a barrier;
    returns their results, raises the first exception a job raised, or WorkerTimeout if a thread has not returned after `timeout`
    seconds -- and then refuses every later call, so that nothing more is started behind a thread that hangs."""

    def __init__(self, n=2):
        self.n, self.hung, self.threads, self.inbox = n, False, [], [queue.Queue() for _ in range(n)]

    def _serve(self, i):
        while True:
            job, barrier, box, done = self.inbox[i].get()
            try:
                barrier.wait()
                box[i] = (True, job())
            except BaseException as e:      # noqa: BLE001 (handed to the caller)
                box[i] = (False, e)
            finally:
                done[i].set()

    def run(self, jobs, timeout):
        if self.hung:
            raise WorkerTimeout('a worker thread did not return from an earlier job: nothing more is started')
        assert len(jobs) == self.n
        if not self.threads:
            self.threads = [threading.Thread(target=self._serve, args=(i,), daemon=True, name=f'reentrancy-{i}') for i in range(self.n)]
            for t in self.threads:
                t.start()
        barrier, box, done = threading.Barrier(self.n, timeout=timeout), [None] * self.n, [threading.Event() for _ in range(self.n)]
        for i, job in enumerate(jobs):
            self.inbox[i].put((job, barrier, box, done))
        for i in range(self.n):
            if not done[i].wait(timeout):
                self.hung = True
                raise WorkerTimeout(f'thread {i} has not returned after {timeout} s')
        for ok, value in box:
            if not ok:
                raise value
        return [value for _, value in box]


# ---- pairs that are not run together ---------------------------------------------------------------------------------------------
# entry point -> the header sentence that says it waits for its stream: a case that makes such a call cannot be queued behind a closed
# gate from one thread (the call would sit out the gate) and runs from two threads only.  Taken from stream_order.SYNC_DOCUMENTED.
def waiting_calls():
    fns = SO.abi_stream_functions()
    return {f: sentence for f, sentence in SO.SYNC_DOCUMENTED.items() if f in fns}


# ... unless the wait is the case's closing status read, whose answer steers nothing: it is deferred until the gate is open
DEFERRED_STATUS = {'rohm_posenet_exchange_status': ('posenet_forward', 'posenet_loop')}
# case family -> the waiting call its cases make (the sentence is waiting_calls()'s); the clip-resident loops are in NOT_TOGETHER
TWO_THREADS_ONLY = {
    'posenet_guided': 'rohm_posenet_exchange_status',       # the guided step polls the status after its forward and acts on the answer
    'track_resample': 'rohm_track_resample',
    'floor': 'rohm_floor_hypotheses',
}

_WHOLE_DEVICE = ('the stream-K output head and the clip-resident TrajNet step launch 256 one-per-CU workgroups that meet through L2, so two '
                 'of them in flight on two streams cannot both be resident')
# a substring of the case name -> (what the launch asks for, read in the sources; the header sentence that says two do not fit)
NOT_TOGETHER = {
    'output_process[B32]': ('gemm_f32.hip launch_one: kSkWorkgroups = 256 workgroups with 84 KiB of LDS each, one per CU; a workgroup '
                            'that holds a tile\'s tail waits for the workgroup that holds its head', _WHOLE_DEVICE),
    'resident 1': ('trajnet_resident.hip: kNumXCD * kWG = 8 x 32 = 256 workgroups per step, all 32 of an XCD meet after every layer '
                   '(xcd_sync)', _WHOLE_DEVICE),
}
# cases that cannot be run from two threads for a reason of the CASE, not of the library (tests/test_gpu_stale_memory.py)
THREAD_EXEMPT = {
    'clips_repr[C2, L16, joint noise]': 'the case patches torch\'s allocators itself (stale_memory.poison around its inputs): two '
                                        'threads would undo each other\'s patch',
    'posenet_train[L1, B2, T63, dropout 0.1]': 'the dropout seed is drawn from torch\'s process-wide CPU generator after torch.manual_seed',
    'posenet_train[L1, B2, T143, dropout 0.1]': 'the dropout seed is drawn from torch\'s process-wide CPU generator after torch.manual_seed',
}


def not_together(case):
    """(key, reason, header sentence) if two runs of `case` may not be in flight together, else None."""
    for key, (reason, sentence) in NOT_TOGETHER.items():
        if key in case:
            return key, reason, sentence
    return None
