"""GPU: every wait-free entry point records into a graph and replays (include/rohm_hip.h, "Conventions": recordable calls).

tests/test_gpu_stale_memory.py, tests/test_gpu_bounds.py and tests/test_gpu_stream_order.py hold the entry points to the header's
conventions in eager calls.  A replay is where a wait-free call can still be silently wrong: a recorded copy from the caller's host
array reads whatever that array has become, a decision taken once on the host is not a node, a second stream may not be joined.
Here every case follows the protocol of tests/graph_replay.py (`run_case`: eager E1 / E2 / E11 on a side stream after one warm-up
call, record on value set 1 under all-ones poison, rewrite and drop every host array, replay on sets 1, 2, 1 over poisoned outputs
and workspaces, two replays in a row for in-place operands, the call log, the exchange status), BIT FOR BIT against the same call
made eagerly.  Cases call through the Python wrappers wherever those are free of waits when handed device tensors; where a wrapper
waits in Python right after its launch (it reads sums back, or uploads an index list) the entry point is recorded through
rohm_amd._lib and the case says so: rohm_amass_preprocess, rohm_amass_metrics, rohm_scene_metrics, rohm_traj_report,
rohm_track_quality.  What a wrapper allocates while recording comes from the graph's own pool and is filled with all-ones bytes by
a RECORDED fill; buffers that exist before the capture (a handle's cached workspace, the case's own outputs and scratch) are
poisoned between replays.  Together graph_replay.REPLAYED (75 entry points, 29 cases) and REFUSED_WHILE_RECORDING (3) are the
public headers' 78 stream-taking functions; EXEMPT is empty, and the call logs hold REPLAYED to the truth family by family.
The cases of rohm_multiview.h, rohm_fit_views.h and rohm_rig.h are those of tests/header_cases.py, value sets 7 and 8 in the slots.
Several families of stale_memory.COVERAGE share one case on purpose where their entry points feed one another or share their
inputs (ops: GEMM, LayerNorm GEMM, output head, attention; render: depth -> probe -> mask, normals -> colour; data: the ten
data-side calls of one recording; metrics; track): one graph of 7 - 35 nodes instead of ten, and the entry points are recorded in
the order and on the buffers in which the loaders use them.  The price: a failure names the output label, not a case of its own,
and no entry point of these is instantiated as a graph by itself.

The check can fail (run first, no library code): a torch chain whose middle step reads a Python float recorded by value fails
"replay on value set 2"; a fake entry point that is never called while recording fails check 6 by name; and a hipMemcpyAsync from
a PAGEABLE host array, recorded and then rewritten, shows what this runtime does -- MEASURED on MI355X: the call is accepted and
the replay delivers the NEW contents (PAGEABLE_COPY_REPLAYS = 'new'): the node keeps the host pointer, nothing is staged at the
call, whereas eagerly the same copy is staged (tests/test_gpu_stream_order.py).  The same was checked once against the library
itself, in an experiment copy with launch_time_path_steps put back to its recorded copy and the host arrays kept alive: both
TrajNet loop cases tried failed at "first replay" (x element 0: -0.6316 replayed, -0.6174 eager at 130 steps), their neighbour
trajnet[forward] passed.

Refusals: rohm_track_resample, rohm_floor_hypotheses and rohm_posenet_exchange_status wait for their stream; on a recording stream
each returns ROHM_ERR_UNSUPPORTED with its name in rohm_last_error before it issues anything, and the capture -- which holds a
marker fill before and an add after the refused call -- ends and replays.  (They synchronised unconditionally before this module;
the refusals were added by reading, the un-fixed wait was never run under a capture.)

Findings (fixed in the same change):
  * rohm_trajnet_sample_loop uploaded the timesteps of every run of 128 steps with hipMemcpyAsync straight from the caller's
    `t_model` (csrc/trajnet.hip, launch_time_path_steps).  Recorded, the copy node keeps the HOST POINTER and every replay reads
    what the wrapper's array has become (a freed numpy array, in rohm_amd).  The timesteps now travel by value in the arguments of
    the time-path launch: no upload at all, nothing recorded points at caller host memory.  `trajnet[loop, TrajNet, 130 steps]`
    rewrites `t_model` after the capture for this; its second run of steps starts at t_model + 128.
  * TrajControl's control stream and its five events were created lazily inside the first loop call of a thread, also when that call
    was being recorded.  They are no longer created under a capture: such a graph takes the one-stream order (bit-identical).  With
    the stream in place (every case makes a warm-up call) the recorded graph has the parallel branch, joined through the events the
    eager path uses, and replays bit-equal to the one-stream graph: no change was needed there.  That the two graphs differ is
    asserted on their structure (`graph_shape`): the one-stream capture is a chain, 440 nodes and 439 edges; with the control
    stream 434 nodes, 439 edges and 6 nodes with two out-edges.
  * rohm_amd.optim.AdamW.step() and PoseNet.forward (train mode, dropout > 0) froze a host scalar -- the step count, the dropout
    seed -- into a graph without a word; both raise now while the current stream records.  At the C ABI a replay repeats the
    recorded `step` / `seed`; the header says so.
  * nothing else: first-call work (exchange arming, pad clears, the cond hoist, launch plans) is recorded as nodes or is a pure host
    decision on sizes; every replay over poisoned workspaces matched.

What stays unseen -- nobody should take it for covered:
  * host arrays that wrappers build themselves and the test cannot reach (the weight structs of the training calls, the item list of
    rohm_result_rows, camera and transform tables of the renderers): they go out of scope when the wrapper returns, but are not
    REWRITTEN first.  Reached and rewritten: t_model and coef of both loops, K and k of rohm_keypoints_undistort, the pointer and
    numel tables of rohm_grad_norm / rohm_adamw_step;
  * anything after a refusal inside the same call;
  * recording with the launch profiler on (outside the contract);
  * the first-ever call of a process made under a capture: every case makes one eager warm-up call first (torch asks for that of
    any captured code; the header requires none for correctness);
  * the clip-resident TrajNet loop: it waits, so under a capture it steps aside (asserted: rohm_trajnet_loop_mode() == 0 for the
    recording call) and the launch-per-layer form is what replays.

Numbers (MI355X, the default environment: four hardware queues, nothing set).  29 cases, 29 graphs of the cases plus 10 small ones
(the three planted checks, three refusals, the pageable copy, three Python-layer refusals), 117 replays by the cases, 10797 nodes in
the cases' graphs (hipGraphGetNodes on the kept graph; the three header cases: 13 / 8 / 20 nodes, 5 - 9 ms each).  The 130-step TrajNet graph: 7704 nodes in one chain (no fork), capture
0.009 s, instantiation 0.007 s (timed by itself, `CUDAGraph.instantiate()`); the other graphs 1 - 781 nodes, capture 0.001 - 0.021 s,
instantiation at most 0.006 s (the forked TrajControl graph) -- so the long graph is not slow to instantiate; its whole case takes
0.44 s.  Slowest case: train[TrajControl, B2, T16], 781 nodes, 0.9 - 1.1 s in run_case (1.7 s as a test, with the module's set-up);
all cases 3.4 s.  Wall time of the whole module, 36 tests, run alone: 11.1 s; with the three header cases, 39 tests, after the other
three families in one process: all cases 2.5 s, 6.6 s summed over its tests."""
import ctypes as C

import numpy as np
import pytest
import torch

import graph_replay as GR
import header_cases as HC
import stale_memory as SM
import stream_order as SO
import test_gpu_stale_memory as G
from helpers import seeded

pytestmark = pytest.mark.gpu
DEV = G.DEV
# what a replay of a recorded asynchronous copy from pageable host memory reads after the array was rewritten, as measured:
# 'old' (staged at the call), 'new' (the node keeps the host pointer) or 'refused' (the runtime does not record such a copy)
PAGEABLE_COPY_REPLAYS = 'new'

_SIDE = []


def _side():
    if not _SIDE:
        _SIDE.append(torch.cuda.Stream())
    return _SIDE[0]


def _lib():
    from rohm_amd import _lib
    return _lib.lib()


def _two(slots, name, make):
    """A slot whose value sets are make(0) and make(1)."""
    return slots.add(name, make(0), make(1))


def _nothing(h):
    pass


# ================================================================================================ the check can fail
class _HostScalarSlots(GR.Slots):
    """Slots that also move a Python float with the value set: what a call reads of it while recording is recorded BY VALUE."""

    def __init__(self, device, box):
        super().__init__(device)
        self.box = box

    def load(self, k):
        super().load(k)
        self.box['k'] = 1.5 * k


def _chain_case(box):
    s = _HostScalarSlots(DEV, box)
    _two(s, 'a', lambda k: seeded(1 + k, 4096))

    def call(s, h):
        b = torch.empty_like(s['a'])
        torch.mul(s['a'], 2.0, out=b)
        c = torch.empty_like(b)
        torch.add(b, box['k'], out=c)               # a Python float: eager it follows the value set, recorded it is frozen
        d = torch.empty_like(c)
        torch.mul(c, 3.0, out=d)
        return [('d', d)]
    return s, call


def test_a_host_scalar_recorded_by_value_is_reported():
    s, call = _chain_case({'k': 0.0})
    with pytest.raises(AssertionError, match='replay on value set 2'):
        GR.run_case(s, call, dict, _nothing, _side(), claims=(), lib_obj=object(), stream_at={})
    torch.cuda.synchronize()


def test_a_recorded_copy_from_pageable_host_memory_is_measured():
    """hipMemcpyAsync(device, pageable host array, host to device) recorded into a graph; the array is rewritten afterwards, the
    graph replayed.  MEASURED on MI355X (ROCm 7): the replay delivers PAGEABLE_COPY_REPLAYS.  This is the measurement the TrajNet
    130-step case rests on: eager, the same copy is staged at the call."""
    hip = _hip_runtime()
    hip.hipMemcpyAsync.restype = C.c_int
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    host = np.arange(128, dtype=np.int64)
    old = host.copy()
    dst = torch.full((128,), -1, dtype=torch.int64, device=DEV)
    side, graph, rc = _side(), torch.cuda.CUDAGraph(), None
    torch.cuda.synchronize()
    try:
        with torch.cuda.graph(graph, stream=side):
            rc = hip.hipMemcpyAsync(dst.data_ptr(), host.ctypes.data, host.nbytes, 1, C.c_void_p(side.cuda_stream))
    except RuntimeError as e:                       # the runtime refused the copy and with it the capture
        print('capture failed:', e)
        outcome = 'refused'
    else:
        if rc != 0:
            outcome = 'refused'
        else:
            host[:] = 1000 + old                    # other valid values; the array stays alive, so a stale read is a defined read
            graph.replay()
            torch.cuda.synchronize()
            got = dst.cpu().numpy()
            outcome = 'old' if (got == old).all() else 'new' if (got == host).all() else f'neither: {got[:4]}'
    print('a recorded pageable host-to-device copy replays:', outcome, '(hipMemcpyAsync returned', rc, ')')
    assert outcome == PAGEABLE_COPY_REPLAYS


def _hip_runtime():
    """The HIP runtime this process has ALREADY loaded (torch's), by its path: a second copy would be another runtime."""
    with open('/proc/self/maps') as f:
        paths = sorted({line.split()[-1] for line in f if 'libamdhip64' in line})
    assert paths, 'no HIP runtime is loaded'
    return C.CDLL(paths[0])


def graph_shape(graph):
    """(nodes, edges, forks) of a kept torch.cuda.CUDAGraph, from the HIP runtime (hipGraphGetNodes / hipGraphGetEdges on
    `raw_cuda_graph()`): forks = nodes with more than one out-edge.  A capture of ONE stream is a chain: edges = nodes - 1, no fork."""
    hip = _hip_runtime()
    raw = C.c_void_p(graph.raw_cuda_graph())
    n, e = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipGraphGetNodes(raw, None, C.byref(n)) == 0 and hip.hipGraphGetEdges(raw, None, None, C.byref(e)) == 0
    src, dst = (C.c_void_p * max(e.value, 1))(), (C.c_void_p * max(e.value, 1))()
    got = C.c_size_t(e.value)
    assert hip.hipGraphGetEdges(raw, src, dst, C.byref(got)) == 0 and got.value == e.value
    out_degree = {}
    for i in range(e.value):
        out_degree[src[i]] = out_degree.get(src[i], 0) + 1
    return n.value, e.value, sum(1 for d in out_degree.values() if d > 1)


class _StandIn:
    def rohm_fake_launch(self, x, stream):
        x.mul_(2.0)
        return 0


def test_an_entry_point_never_called_while_recording_fails_by_name():
    s = GR.Slots(DEV)
    _two(s, 'a', lambda k: seeded(3 + k, 64))

    def call(s, h):
        return [('b', s['a'] * 2.0)]
    with pytest.raises(AssertionError, match='never called while the stream was recording.*rohm_fake_launch'):
        GR.run_case(s, call, dict, _nothing, _side(), claims=['rohm_fake_launch'], lib_obj=_StandIn(), stream_at={'rohm_fake_launch': 1})
    torch.cuda.synchronize()


# ================================================================================================ refusals
def _refusal(name, call):
    """A graph that holds a marker fill; `call()` -> rc of the refused function on the recording stream."""
    lib = _lib()
    side, graph = _side(), torch.cuda.CUDAGraph()
    flag = torch.zeros(4, device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        flag.fill_(7.0)
        rc = call()
        msg = lib.rohm_last_error()
        flag.add_(1.0)
    assert rc == -4, (name, rc, msg)                                # ROHM_ERR_UNSUPPORTED
    assert msg and name.encode() in msg, (name, msg)
    graph.replay()                                                  # the capture survived the refused call
    torch.cuda.synchronize()
    assert flag.tolist() == [8.0] * 4


def test_track_resample_is_refused_while_recording():
    from rohm_amd._lib import ptr, stream_ptr
    N, n_out = 8, 6
    times = torch.linspace(0.0, 0.35, N, dtype=torch.float64, device=DEV)
    valid = torch.arange(N, dtype=torch.int32, device=DEV)
    params = torch.zeros(N, 79, dtype=torch.float64, device=DEV)
    times_dst = torch.linspace(0.0, 0.3, n_out, dtype=torch.float64, device=DEV)
    params_out = torch.zeros(n_out, 79, dtype=torch.float64, device=DEV)
    src_index, gap = torch.zeros(n_out, 2, dtype=torch.int32, device=DEV), torch.zeros(n_out, dtype=torch.uint8, device=DEV)
    _refusal('rohm_track_resample', lambda: _lib().rohm_track_resample(
        ptr(times), ptr(valid), ptr(params), None, None, ptr(times_dst), 0.2, N, N, 0, 0, n_out, ptr(params_out), None, None,
        ptr(src_index), ptr(gap), stream_ptr(DEV)))


def test_floor_hypotheses_is_refused_while_recording():
    from rohm_amd._lib import ptr, stream_ptr
    P, K = 8, 4
    points = seeded(1, P, 3).to(DEV)
    triples = torch.tensor([[0, 1, 2], [1, 2, 3], [4, 5, 6], [5, 6, 7]], dtype=torch.int32, device=DEV)
    planes = torch.zeros(K, 4, dtype=torch.float64, device=DEV)
    scores, best = torch.zeros(K, dtype=torch.int64, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    _refusal('rohm_floor_hypotheses', lambda: _lib().rohm_floor_hypotheses(
        ptr(points), P, None, 0, ptr(triples), K, 0.05, 0.02, ptr(planes), ptr(scores), ptr(best), stream_ptr(DEV)))


def test_posenet_exchange_status_is_refused_while_recording():
    from rohm_amd._lib import ptr, stream_ptr
    net = G._make_posenet('0')
    B, T = 2, 143
    with torch.cuda.stream(_side()):
        nat = net.native(torch.device(DEV))
        ws = nat.workspace(B, T)
    _refusal('rohm_posenet_exchange_status', lambda: _lib().rohm_posenet_exchange_status(nat.handle, B, T, ptr(ws), ws.numel(), stream_ptr(DEV)))


# ================================================================================================ the cases
CASES = {}              # name ('family[variant]') -> thunk that runs the protocol and returns run_case's dict
_RESULTS = {}


def case(name):
    def deco(fn):
        assert name not in CASES
        CASES[name] = fn
        return fn
    return deco


_HIP_ERROR = []         # the first case that met an error of the HIP runtime: nothing more is started on the GPU after it


def _is_hip_error(e):
    text = f'{type(e).__name__}: {e}'
    return any(w in text for w in ('HIP error', 'hipError', 'illegal memory access', 'AcceleratorError', 'HSA_STATUS'))


def _result(name):
    if name not in _RESULTS:
        if _HIP_ERROR:
            _RESULTS[name] = RuntimeError(f'{name} was not run: {_HIP_ERROR[0]} met an error of the HIP runtime before it')
            return _RESULTS[name]
        try:
            _RESULTS[name] = CASES[name]()
            torch.cuda.synchronize()
            _RESULTS[name]['shape'] = graph_shape(_RESULTS[name]['graph'])
        except Exception as e:                  # kept for the case's own test; the coverage test goes on unless the runtime failed
            _RESULTS[name] = e
            if _is_hip_error(e):
                _HIP_ERROR.append(name)
    return _RESULTS[name]


# ---- the building blocks ------------------------------------------------------------------------------------------------------------
@case('ops[gemm, gemm_res_layernorm, output_process, attention]')
def _ops():
    import math
    from rohm_amd import ops
    s = GR.Slots(DEV)
    M, N, K = 288, 512, 64                      # 8 column tiles of 64: the tiles really exchange (tests/test_gpu_stale_memory.py)
    _two(s, 'a', lambda k: seeded(M + N + 50 * k, M, K))
    _two(s, 'w', lambda k: seeded(K + 7 + 50 * k, N, K) / math.sqrt(K))
    _two(s, 'bias', lambda k: seeded(3 + 50 * k, N))
    _two(s, 'res', lambda k: seeded(4 + 50 * k, M, N) * 2 + 0.3)
    _two(s, 'g', lambda k: seeded(5 + 50 * k, N) * 0.5 + 1.0)
    _two(s, 'b', lambda k: seeded(6 + 50 * k, N))
    B, T, D, Cc = 32, 143, 512, 272             # 32: the smallest stream-K plan of the output head
    _two(s, 'h', lambda k: seeded(B + 50 * k, B * (T + 1), D) * 2 + 0.1)
    _two(s, 'hw', lambda k: seeded(B + 1 + 50 * k, Cc, D) / math.sqrt(D))
    _two(s, 'hb', lambda k: seeded(B + 2 + 50 * k, Cc))
    _two(s, 'qkv', lambda k: seeded(7 + 50 * k, 144, 3 * 4 * 128))
    keep = {}

    def call(s, h):
        out = [('gemm', ops.gemm(s['a'], s['w'], s['bias']))]
        ln, keep['ln scratch'] = ops.gemm_res_layernorm(s['a'], s['w'], s['bias'], s['res'], s['g'], s['b'], return_scratch=True)
        head, keep['head scratch'] = ops.output_process(s['h'], s['hw'], s['hb'], B, T, ch_off=22, c_total=294, return_scratch=True)
        return out + [('gemm_res_layernorm', ln), ('output_process', head), ('attention', ops.attention(s['qkv'], 1, 4))]

    def status():
        torch.cuda.synchronize()
        assert int(keep['ln scratch'][0]) == 0 and int(keep['head scratch'][0]) == 0, 'exchange error word'
    return GR.run_case(s, call, dict, _nothing, _side(), status=status,
                       claims=['rohm_gemm_f32', 'rohm_gemm_res_layernorm_f32', 'rohm_output_process_f32', 'rohm_attention_f32'])


@case('ops[layernorm, in place]')
def _layernorm():
    from rohm_amd import ops
    s = GR.Slots(DEV)
    _two(s, 'x', lambda k: seeded(9 + k, 144, 512) * 3 + 0.5)
    _two(s, 'g', lambda k: seeded(1 + 10 * k, 512))
    _two(s, 'b', lambda k: seeded(2 + 10 * k, 512))
    return GR.run_case(s, lambda s, h: [('x', ops.layernorm_(s['x'], s['g'], s['b']))], dict, _nothing, _side(), inplace=True,
                       claims=['rohm_layernorm_f32'])


@case('planes[mode 16]')
def _planes():
    """tests/test_gpu_stale_memory.py::_planes with its inputs in slots; layernorm_planes_ works in place."""
    import math
    from rohm_amd import ops
    mode, M, N, K, ws = 16, 144, 512, 512, 256.0
    s = GR.Slots(DEV)
    host_a = [seeded(M + N + 50 * k, M, K) for k in (0, 1)]
    host_w = [seeded(K + 7 + 50 * k, N, K) / math.sqrt(K) for k in (0, 1)]
    s.add('a', *host_a)
    s.add('w', *host_w)
    _two(s, 'bias', lambda k: seeded(3 + 50 * k, N))
    _two(s, 'res', lambda k: seeded(4 + 50 * k, M, N))

    def stats(a):
        g = a.double().reshape(M // 16, 16, K // 16, 16)
        return torch.stack([g.sum(-1), (g * g).sum(-1)], -1).permute(0, 2, 1, 3).contiguous().float()
    s.add('stats', *[stats(a) for a in host_a])
    s.add('ln_c', *[w.sum(1) for w in host_w])
    _two(s, 'x', lambda k: seeded(5 + 50 * k, M, 512) * 3 + 0.5)
    _two(s, 'g', lambda k: seeded(1 + 50 * k, 512))
    _two(s, 'b', lambda k: seeded(2 + 50 * k, 512))
    _two(s, 'qkv', lambda k: seeded(7 + 50 * k, 144, 3 * 4 * 128))

    def call(s, h):
        ap, wp = ops.planes_split(s['a'], mode), ops.planes_split(s['w'], mode, scale=ws)
        out = [('a planes', ap), ('w planes', wp)]
        c, cp = ops.gemm_planes(ap, wp, M, N, K, mode, s['bias'], None, 1, out_planes=True, acc_scale=1.0 / ws)
        out += [('gelu gemm', c), ('gelu gemm planes', cp)]
        c2, cp2, st = ops.gemm_planes_ln(ap, wp, M, N, K, mode, s['bias'], s['res'], 2, acc_scale=1.0 / ws, want_stats=True, ln_dim=N,
                                         out_planes=True)
        out += [('ln producer', c2), ('ln producer planes', cp2), ('ln producer stats', st)]
        c3, _, _ = ops.gemm_planes_ln(ap, wp, M, N, K, mode, s['bias'], None, 1, acc_scale=1.0 / ws, ln_stats=s['stats'], ln_c=s['ln_c'],
                                      ln_dim=K)
        out += [('ln consumer', c3)]
        out += [('layernorm planes', ops.layernorm_planes_(s['x'], s['g'], s['b'], mode)), ('layernorm', s['x'])]
        return out + [('attention planes', ops.attention_planes(s['qkv'], 1, 4, mode))]
    return GR.run_case(s, call, dict, _nothing, _side(), inplace=True,
                       claims=['rohm_planes_split', 'rohm_gemm_planes', 'rohm_gemm_planes_ln', 'rohm_layernorm_planes_f32',
                               'rohm_attention_planes_f32'])


@case('ddpm[step, table, q_sample, dropout mask]')
def _ddpm():
    from rohm_amd import ops
    from rohm_amd.model.posenet import dropout_mask
    from test_gpu_posenet import make_diffusion
    B = 3
    s = GR.Slots(DEV)
    for i, name in enumerate(('x', 'x0', 'nz', 'ga')):
        _two(s, name, lambda k, i=i: seeded(1 + i + 20 * k, B, 294, 1, 143))
    _two(s, 'tables', lambda k: seeded(5 + 20 * k, 10, 4))
    s.add('t', torch.tensor([0, 9, 4]), torch.tensor([3, 1, 7]))                    # indices into the 10 rows of `tables`
    s.add('tq', torch.tensor([0, 500, 999]), torch.tensor([10, 3, 700]))            # ... and into the 1000 steps of the schedule
    diff = make_diffusion(1000)

    def call(s, h):
        return [('ddpm_step', ops.ddpm_step(s['x'], s['x0'], s['nz'], 0.3, 0.7, 0.1, grad=s['ga'], grad_scale=2.0)),
                ('ddpm_step_table', ops.ddpm_step_table(s['x'], s['x0'], s['nz'], s['tables'], s['t'], grad_a=s['ga'], w_a=3.0)),
                ('q_sample', diff.q_sample(s['x0'], s['tq'], noise=s['nz'])),
                ('dropout mask', dropout_mask(1234, 0, 2, (2, 64, 512), 0.1, DEV).to(torch.uint8))]
    return GR.run_case(s, call, dict, _nothing, _side(),
                       claims=['rohm_ddpm_step', 'rohm_ddpm_step_table', 'rohm_q_sample', 'rohm_posenet_dropout_mask'])


# ---- PoseNet ------------------------------------------------------------------------------------------------------------------------
def _posenet_net():
    from test_gpu_posenet import make_posenet
    return make_posenet(5)[0]                   # the released shape: 8 layers, the handle's own launch plan


def _pose_status(net, B, T):
    """(buffers(), status()) of a PoseNet case on the side stream: the cached workspace; a clean exchange status."""
    nat = net.native(torch.device(DEV))

    def buffers():
        return [nat.workspace(B, T)]

    def status():
        with torch.cuda.stream(_side()):
            net.check_exchange()
    return buffers, status


@case('posenet[forward, B2]')
def _posenet_forward():
    net, B, T = _posenet_net(), 2, 143
    s = GR.Slots(DEV)
    _two(s, 'x', lambda k: seeded(1 + 10 * k, B, 294, 1, T))
    _two(s, 'c', lambda k: seeded(2 + 10 * k, B, 294, 1, T))
    s.add('t', torch.tensor([1, 38]), torch.tensor([999, 0]))
    buffers, status = _pose_status(net, B, T)
    return GR.run_case(s, lambda s, h: [('out', net({'x_t': s['x'], 'cond': s['c']}, s['t']))], dict, _nothing, _side(),
                       buffers=buffers, status=status, claims=['rohm_posenet_forward'])


def _posenet_loop(B, n=4):
    """rohm_posenet_sample_loop, n_steps = 4 (the smallest with the cond hoist), x0_last and x_in_last, noise, the last sigma 0.  B = 2:
    a launch per GEMM; B = 32: stack launches with their closing phase and the folded in-projection."""
    net, T = _posenet_net(), 143
    s = GR.Slots(DEV)
    _two(s, 'x', lambda k: seeded(1 + 10 * k, B, 294, 1, T))
    _two(s, 'c', lambda k: seeded(2 + 10 * k, B, 294, 1, T))
    _two(s, 'noise', lambda k: seeded(3 + 10 * k, n, B, 294, 1, T))
    x_in = torch.zeros(B, 294, 1, T, device=DEV)

    def host():
        coef = np.asarray([[0.05 + 0.01 * i, 0.95 - 0.01 * i, 0.1] for i in range(n)], np.float32)
        coef[n - 1, 2] = 0.0
        return dict(t=np.asarray([400 - 3 * i for i in range(n)], np.int64), coef=coef)

    def rewrite(h):
        GR.rewrite_valid(h['t'], 0, 999)
        GR.rewrite_valid(h['coef'], 0.0, 1.0)

    def call(s, h):
        x0 = net.sample_loop_native(s['x'], s['c'], h['t'], h['coef'], s['noise'], want_x0_last=True, x_in_last=x_in)
        return [('x', s['x']), ('x0 of the last step', x0), ('input of the last step', x_in)]
    buffers, status = _pose_status(net, B, T)
    r = GR.run_case(s, call, host, rewrite, _side(), inplace=True, buffers=buffers, status=status, claims=['rohm_posenet_sample_loop'])
    # the pass counter lives in the workspace and is advanced on the device: every replay draws fresh tags
    nat = net.native(torch.device(DEV))
    off = _lib().rohm_posenet_status_offset(nat.handle, B, T)
    passes = []
    with torch.cuda.stream(_side()):
        word = buffers()[0][off:off + 12].view(torch.int32)          # (the workspace is cached per stream: ask on the side stream)
        s.load(1)
        for _ in range(3):
            r['graph'].replay()
            r['replays'] += 1
            _side().synchronize()
            passes.append(int(word[2]))
    steps = (passes[1] - passes[0], passes[2] - passes[1])
    print(f'posenet loop B{B}: pass counter after three more replays {passes}, exchange mode {nat.exchange_mode}')
    # One pass per step: the x_t pack of step 0 and the finish-and-pack kernel of every later step each advance the counter by one
    # (n per replay).  Where the steps are stack launches that close themselves (B = 32), only the pack of step 0 touches the
    # counter: it adds 1 and what the LAST step of the replay before left pending, pass_add + 1 = n -- n + 1 per replay.
    stacked = B >= 32 and nat.exchange_mode & 3 == 3
    assert steps == ((n + 1, n + 1) if stacked else (n, n)), (passes, nat.exchange_mode)
    assert int(word[0]) == 0
    status()
    return r


case('posenet[loop, B2, 4 steps]')(lambda: _posenet_loop(2))
case('posenet[loop, B32, 4 steps]')(lambda: _posenet_loop(32))


# ---- TrajNet ------------------------------------------------------------------------------------------------------------------------
def _traj_slots(B, T):
    s = GR.Slots(DEV)
    _two(s, 'x', lambda k: seeded(1 + 10 * k, B, T, 13))
    _two(s, 'c', lambda k: seeded(2 + 10 * k, B, T, 13))
    _two(s, 'ctl', lambda k: seeded(3 + 10 * k, B, T, 272))
    return s


def _traj_buffers(net, B, T):
    nat = net.native(torch.device(DEV))
    return lambda: [nat.workspace(B, T)]


def _trajnet_forward(ctrl):
    net, B, T = G._make_trajnet(ctrl), 2, 16
    s = _traj_slots(B, T)
    s.add('t', torch.tensor([3, 40]), torch.tensor([77, 5]))
    return GR.run_case(s, lambda s, h: [('out', net({'x_t': s['x'], 'cond': s['c'], 'control_cond': s['ctl']}, s['t']))], dict, _nothing,
                       _side(), buffers=_traj_buffers(net, B, T), claims=['rohm_trajnet_forward'])


case('trajnet[forward, TrajNet, B2, T16]')(lambda: _trajnet_forward(False))
case('trajnet[forward, TrajControl, B2, T16]')(lambda: _trajnet_forward(True))


def _trajnet_loop(ctrl, n, env):
    """rohm_trajnet_sample_loop recorded with the environment's default form allowed: under a capture the clip-resident form steps
    aside by itself (rohm_trajnet_loop_mode() == 0 for the recording call); the eager calls are held to the same launch-per-layer form
    by ROHM_TRAJ_RESIDENT=0."""
    net, B, T = G._make_trajnet(ctrl), 2, 16
    s = _traj_slots(B, T)
    _two(s, 'noise', lambda k: seeded(4 + 10 * k, n, B, T, 13))
    x_in = torch.zeros(B, T, 13, device=DEV)

    def host():
        coef = np.asarray([[0.05 + 0.0005 * i, 0.95 - 0.0005 * i, 0.1] for i in range(n)], np.float32)
        coef[n - 1, 2] = 0.0
        return dict(t=np.asarray([99 - (7 * i) % 100 for i in range(n)], np.int64), coef=coef)

    def rewrite(h):                             # the step-2 host rewrite: other valid timesteps and coefficients, NOT a second value set
        GR.rewrite_valid(h['t'], 0, 99)
        GR.rewrite_valid(h['coef'], 0.0, 1.0)

    def call(s, h):
        batch = {'x_t': s['x'], 'cond': s['c'], 'control_cond': s['ctl']}
        x0 = net.sample_loop_native(s['x'], s['c'], h['t'], h['coef'], s['noise'], want_x0_last=True, batch=batch, x_in_last=x_in)
        return [('x', s['x']), ('x0 of the last step', x0), ('input of the last step', x_in)]

    def after_record():
        assert _lib().rohm_trajnet_loop_mode() == 0, 'the recorded loop call did not take the launch-per-layer form'
    with SM.env(**env):
        return GR.run_case(s, call, host, rewrite, _side(), inplace=True, buffers=_traj_buffers(net, B, T), after_record=after_record,
                           eager_env=dict(ROHM_TRAJ_RESIDENT='0'), claims=['rohm_trajnet_sample_loop'])


case('trajnet[loop, TrajControl, control stream, 4 steps]')(lambda: _trajnet_loop(True, 4, dict(ROHM_TRAJ_CTRL_STREAM=None)))
case('trajnet[loop, TrajControl, one stream, 4 steps]')(lambda: _trajnet_loop(True, 4, dict(ROHM_TRAJ_CTRL_STREAM='0')))
case('trajnet[loop, TrajNet, 130 steps]')(lambda: _trajnet_loop(False, 130, {}))


# ---- one training step as one graph -------------------------------------------------------------------------------------------------
def _train_step(kind, p=0.0, seed=4242, step=3):
    """*_train_forward, the loss gradient as a plain torch op, *_train_backward, rohm_grad_norm, rohm_adamw_step with clip_coef, through
    rohm_amd._lib with a fixed `step` (and, for PoseNet with dropout, a fixed seed through the autograd function: PoseNet.forward
    itself refuses to draw a seed while recording).  The parameters and moments are in-place operands: slots whose two value sets are
    the same, so a replay on input set 2 starts from the same parameters as the eager step on set 2."""
    from rohm_amd import _lib
    from rohm_amd.model.posenet import _PoseNetTrain
    lib = _lib.lib()
    B, T = 2, 16
    s = GR.Slots(DEV)
    if kind == 'posenet':
        net = G._make_posenet(None, L=1, dropout=p).train()
        _two(s, 'x', lambda k: seeded(1 + 10 * k, B, 294, 1, T))
        _two(s, 'c', lambda k: seeded(2 + 10 * k, B, 294, 1, T))
        s.add('t', torch.tensor([1, 38]), torch.tensor([999, 0]))
        _two(s, 'target', lambda k: seeded(4 + 10 * k, B, 294, 1, T))
    else:
        net = G._make_trajnet(kind == 'trajcontrol', mid=512, train=True)
        _two(s, 'x', lambda k: seeded(1 + 10 * k, B, T, 13))
        _two(s, 'c', lambda k: seeded(2 + 10 * k, B, T, 13))
        _two(s, 'ctl', lambda k: seeded(3 + 10 * k, B, T, 272))
        s.add('t', torch.tensor([3, 77]), torch.tensor([50, 0]))
        _two(s, 'target', lambda k: seeded(4 + 10 * k, B, T, 13))
    params = net.train_parameters()
    ms, vs = [], []
    for i, q in enumerate(params):
        q.data = s.add(f'param {i}', q.data, q.data)
        m = seeded(500 + i, *q.shape) * 1e-3
        ms.append(s.add(f'exp_avg {i}', m, m))
        vs.append(s.add(f'exp_avg_sq {i}', m * m, m * m))
    numel = [q.numel() for q in params]
    norm_out = torch.zeros(2, device=DEV)
    nbytes = lib.rohm_grad_norm_scratch_bytes(sum(numel), len(params))
    scratch = torch.zeros((nbytes + 7) // 8, dtype=torch.float64, device=DEV)

    def table(tensors):
        return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])

    def call(s, h):
        for q in params:
            q.grad = None
        if kind == 'posenet' and p > 0:
            y = _PoseNetTrain.apply(net, s['x'], s['c'], s['t'], p, seed, *params)
        elif kind == 'posenet':
            y = net({'x_t': s['x'], 'cond': s['c']}, s['t'])
        else:
            y = net({'x_t': s['x'], 'cond': s['c'], 'control_cond': s['ctl']}, s['t'])
        d_out = (y.detach() - s['target']) * (2.0 / y.numel())                  # the gradient of the mean squared error
        y.backward(d_out)
        # a parameter the network does not use gets no gradient and takes no step (TrajControl has such), as in optim.AdamW
        live = [i for i, q in enumerate(params) if q.grad is not None]
        grads = [params[i].grad for i in live]
        assert len(live) > len(params) // 2 and all(g.is_contiguous() and g.dtype == torch.float32 for g in grads)
        h['tables'] = [table([params[i] for i in live]), table(grads), table([ms[i] for i in live]), table([vs[i] for i in live])]
        h['numel'] = (C.c_longlong * len(live))(*[numel[i] for i in live])
        _lib.check(lib.rohm_grad_norm(h['tables'][1], h['numel'], len(live), 0.05, _lib.ptr(norm_out), _lib.ptr(scratch),
                                      scratch.numel() * 8, _lib.stream_ptr(DEV)), 'rohm_grad_norm')
        _lib.check(lib.rohm_adamw_step(*h['tables'], h['numel'], len(live), 1e-2, 0.9, 0.999, 1e-8, 1e-2, step,
                                       C.c_void_p(norm_out.data_ptr() + 4), _lib.stream_ptr(DEV)), 'rohm_adamw_step')
        return ([('out', y.detach()), ('grad norm and clip coefficient', norm_out)] + [(f'grad {i}', g) for i, g in zip(live, grads)] +
                [(f'param {i}', q.data) for i, q in enumerate(params)] + [(f'exp_avg {i}', m) for i, m in enumerate(ms)] +
                [(f'exp_avg_sq {i}', v) for i, v in enumerate(vs)])

    def rewrite(h):
        GR.rewrite_tables(h['tables'], h['numel'])
    fam = 'posenet' if kind == 'posenet' else 'trajnet'
    return GR.run_case(s, call, dict, rewrite, _side(), inplace=True, buffers=lambda: [scratch],
                       claims=[f'rohm_{fam}_train_forward', f'rohm_{fam}_train_backward', 'rohm_grad_norm', 'rohm_adamw_step'])


case('train[PoseNet, L1, B2, T16, dropout 0]')(lambda: _train_step('posenet', 0.0))
case('train[PoseNet, L1, B2, T16, dropout 0.1, fixed seed]')(lambda: _train_step('posenet', 0.1))
case('train[TrajNet, B2, T16]')(lambda: _train_step('trajnet'))
case('train[TrajControl, B2, T16]')(lambda: _train_step('trajcontrol'))


# ---- guidance, body model, representation, export ------------------------------------------------------------------------------------
@case('guided[forward, skating, proj2d, ddpm table, B2]')
def _guided():
    """One guided step as ONE graph: rohm_posenet_forward, the skating gradient (in one call, and as prepare + all-reduce + apply),
    the 2-D projection gradient, rohm_ddpm_step_table with both gradients."""
    from rohm_amd import ops
    from rohm_amd.body_model import native_for
    from rohm_amd.guidance import guide_2d_projection, guide_skating
    from rohm_amd.utils import synth
    net, (mean, std) = G._make_guided()
    net.dataset.cam_R, net.dataset.cam_t = net.dataset.cam_R.to(DEV), net.dataset.cam_t.to(DEV)     # (no upload inside the call)
    B, T = 2, 143
    s = GR.Slots(DEV)
    _two(s, 'motion', lambda k: synth.plausible_motion(30 + k, B, T, mean, std, angle_scale=2.5 if k == 0 else 0.4))
    _two(s, 'cond', lambda k: synth.plausible_motion(40 + k, B, T, mean, std))
    _two(s, 'x', lambda k: synth.plausible_motion(31 + k, B, T, mean, std) + 0.05 * seeded(3 + k, B, 294, 1, T))
    _two(s, 'nz', lambda k: seeded(4 + 10 * k, B, 294, 1, T))
    _two(s, 'tables', lambda k: seeded(5 + 20 * k, 10, 4))
    s.add('ti', torch.tensor([0, 9]), torch.tensor([3, 1]))
    s.add('t', torch.tensor([10, 10]), torch.tensor([40, 7]))
    cams = [synth.synthetic_camera_batch(k, B) for k in (0, 1)]
    for key in cams[0]:
        s.add(key, cams[0][key].float(), cams[1][key].float() * (1.01 if key in ('focal_length', 'camera_center') else 1.0))

    def call(s, h):
        y = net({'x_t': s['x'], 'cond': s['cond']}, s['t'])
        guided = {'pred_xstart': s['motion']}
        net.guidance_group = None
        one = guide_skating(net, {}, guided, None, 'x_0')
        net.guidance_group = lambda t: t                          # prepare + all-reduce (identity) + apply
        sk, counts = guide_skating(net, {}, guided, None, 'x_0', return_counts=True)
        net.guidance_group = None
        p2d = guide_2d_projection(net, {k: s[k] for k in cams[0]}, guided, None, 'x_0')
        step = ops.ddpm_step_table(s['x'], y, s['nz'], s['tables'], s['ti'], grad_a=sk, w_a=3.0, grad_b=p2d, w_b=0.5)
        return [('out', y), ('skating grad', one), ('skating grad, split', sk), ('counts', counts), ('proj2d grad', p2d), ('step', step)]
    buffers, status = _pose_status(net, B, T)
    body_ws = lambda: buffers() + [native_for(net.smplx_model, torch.device(DEV)).workspace(B, T)]
    return GR.run_case(s, call, dict, _nothing, _side(), buffers=body_ws, status=status,
                       claims=['rohm_posenet_forward', 'rohm_guidance_skating_grad', 'rohm_guidance_skating_prepare',
                               'rohm_guidance_skating_apply', 'rohm_guidance_proj2d_grad', 'rohm_ddpm_step_table'])


@case('smplx[forward with vertices, joints, N17]')
def _smplx():
    from rohm_amd.body_model import lbs_forward
    body, nat = G._make_lbs('mfma')
    N = 17                                      # a part-filled second group of 16 and a part-filled tile of 144
    s = GR.Slots(DEV)
    _two(s, 'pose', lambda k: seeded(1 + 10 * k, N, 22, 3) * 0.4)
    _two(s, 'betas', lambda k: seeded(2 + 10 * k, N, 10))
    _two(s, 'transl', lambda k: seeded(3 + 10 * k, N, 3))

    def call(s, h):
        joints, verts = lbs_forward(nat, s['pose'], 0, s['betas'], s['transl'], want_verts=True)
        out = body(betas=s['betas'], global_orient=s['pose'][:, 0], body_pose=s['pose'][:, 1:].reshape(N, 63), transl=s['transl'])
        return [('joints', joints), ('verts', verts), ('joints only', out.joints)]
    return GR.run_case(s, call, dict, _nothing, _side(), buffers=lambda: [nat.lbs_workspace(N)],
                       claims=['rohm_smplx_forward', 'rohm_smplx_joints'])


def _stats_holder(seed=0):
    from helpers import PoseDataset
    from rohm_amd.utils import synth
    mean, std = synth.synthetic_stats(seed)
    return PoseDataset(mean, std), (mean, std)      # an object: its device copies are cached by the first (eager) call


@case('repr[joints, joints vjp, rederive]')
def _repr():
    from rohm_amd.data_loaders import motion_representation as mr
    from rohm_amd.utils import synth
    body = G._body().to(DEV)
    ds, (mean, std) = _stats_holder()
    B, T = 2, 20
    s = GR.Slots(DEV)
    _two(s, 'x', lambda k: synth.plausible_motion(7 + k, B, T, mean, std))
    _two(s, 'dj', lambda k: seeded(9 + k, B, T, 22, 3))
    _two(s, 'cond', lambda k: seeded(5 + k, B, 294, 1, T - 1))

    def call(s, h):
        out = []
        for mode in ('smplx_params', 'joint_abs_traj', 'joint_rel_traj'):
            out += [('joints ' + mode, mr.joints_from_repr(s['x'], mode, smplx_model=body, stats=ds, layout='bc1t')),
                    ('vjp ' + mode, mr.joints_vjp(s['x'], s['dj'], mode, smplx_model=body, stats=ds, layout='bc1t'))]
        xb = s['x'][:, :, 0].permute(0, 2, 1).contiguous()
        out.append(('rederived trajectory', mr.rederive_traj(xb, ds, ds, body)))
        return out + [('rederived into cond', mr.rederive_traj(xb, ds, ds, body, out=s['cond'], out_layout='bc1t'))]
    return GR.run_case(s, call, dict, _nothing, _side(), claims=['rohm_repr_joints', 'rohm_repr_joints_vjp', 'rohm_traj_rederive'])


@case('export[smplx, blend]')
def _export():
    from rohm_amd import ops
    from rohm_amd.body_model import native_for
    from rohm_amd.utils import synth
    body = G._body().to(DEV)
    handle = native_for(body, DEV).handle
    mean, std = synth.synthetic_stats(0)
    mean_d, std_d = torch.from_numpy(mean).to(DEV), torch.from_numpy(std).to(DEV)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    s = GR.Slots(DEV)
    _two(s, 'x', lambda k: synth.plausible_motion(7 + k, 2, 20, mean, std))
    s.add('clip', i32(0, 1, 1, 0, 5), i32(1, 0, 0, 1, 5))                       # clip 5 does not exist: a NaN row
    s.add('row', i32(0, 3, 19, 7, 0), i32(5, 1, 0, 19, 2))
    s.add('clip_b', i32(-1, 0, 0, -1, -1), i32(0, -1, 1, 0, -1))                # < 0: one candidate
    s.add('row_b', i32(0, 4, 18, 0, 0), i32(6, 0, 1, 18, 0))
    s.add('alpha', torch.tensor([0.0, 0.25, 0.5, 0.0, 0.0], dtype=torch.float64), torch.tensor([0.75, 0.0, 1.0, 0.5, 0.0], dtype=torch.float64))

    def transf(k):
        t = torch.eye(4).repeat(2, 1, 1).contiguous()
        t[:, :3, 3] = torch.tensor([0.5, -1.0, 0.25]) * (1 + k)
        return t
    _two(s, 'transf', transf)

    def rigid(k):
        r = torch.eye(4, dtype=torch.float64)
        r[:3, 3] = 0.1 * k
        return r
    _two(s, 'rigid', rigid)

    def call(s, h):
        params, contact = ops.export_smplx(handle, s['x'], 'bc1t', s['clip'], s['row'], transf=s['transf'], rigid=s['rigid'], mean=mean_d, std=std_d)
        bp, bc, dis = ops.export_smplx_blend(handle, s['x'], 'bc1t', s['clip'], s['row'], s['clip_b'], s['row_b'], s['alpha'],
                                             transf=s['transf'], rigid=s['rigid'], mean=mean_d, std=std_d)
        return [('params', params), ('contact', contact), ('blend params', bp), ('blend contact', bc), ('disagree', dis)]
    return GR.run_case(s, call, dict, _nothing, _side(), claims=['rohm_export_smplx', 'rohm_export_smplx_blend'])


# ---- rendering, images, training helpers ---------------------------------------------------------------------------------------------
@case('render[depth, probe, project, occlusion mask, normals, colour, skeleton]')
def _render():
    """The scene of tests/test_gpu_stale_memory.py; value set 2 moves the vertices and REVERSES the face list (other valid faces, with
    the adjacency that belongs to them)."""
    from rohm_amd import occlusion, render
    verts, faces, cam, size = G._scene()
    faces = np.ascontiguousarray(np.asarray(faces).astype(np.int32).reshape(-1, 3))
    V = verts.shape[1]
    s = GR.Slots(DEV)
    s.add('verts', verts, verts + torch.tensor([0.05, 0.0, 0.1], device=DEV))
    face_sets = [faces, np.ascontiguousarray(faces[::-1])]
    s.add('faces', *[torch.from_numpy(f) for f in face_sets])
    adj = [render.vertex_adjacency(f, V) for f in face_sets]
    s.add('off', *[torch.as_tensor(np.asarray(a[0])).to(torch.int32) for a in adj])
    s.add('ids', *[torch.as_tensor(np.asarray(a[1])).to(torch.int32) for a in adj])
    _two(s, 'colors', lambda k: (seeded(1 + k, V, 4).abs() * 100).clamp(0, 255).to(torch.uint8))
    _two(s, 'joints', lambda k: seeded(1 + 10 * k, 2, 25, 3) * torch.tensor([1.5, 0.8, 0.5]) + torch.tensor([0.0, 0.0, 2.5]))
    _two(s, 'skeleton joints', lambda k: seeded(2 + 10 * k, 3, 22, 3))
    limbs = torch.tensor(np.asarray(render.LIMBS_BODY_SMPL, dtype=np.int32), device=DEV).reshape(-1, 2)
    _two(s, 'hide', lambda k: (seeded(3 + 10 * k, 3, 22 + limbs.shape[0]) > 1.0).to(torch.uint8))
    sphere, cyl = (torch.as_tensor(np.asarray(m[0], dtype=np.float32)).to(DEV) for m in (render.icosphere(1), render.cylinder(8)))
    dist = [0.052, -0.044, 0.0009, 0.0016, 0.003]
    K = occlusion.camera_matrix(cam)

    def call(s, h):
        depth = occlusion.depth_render(s['verts'], s['faces'], cam, size)
        culled = occlusion.depth_render(s['verts'][0], s['faces'], cam, size, cull_backfaces=True)
        pix = occlusion.project_pixels(s['joints'], K, dist)
        probe = occlusion.depth_probe(s['verts'], s['faces'], pix, cam, size)
        mask = occlusion.mask_from_depths(s['joints'], depth[0], probe, K)
        normals = render.vertex_normals(s['verts'], s['faces'], adjacency=(s['off'], s['ids']))
        rgba, d2, fid = render.color_render(s['verts'], s['faces'], s['colors'], cam, size, normals=normals, with_depth=True, with_face_id=True)
        skel = render.skeleton_mesh(s['skeleton joints'], sphere, cyl, limbs=limbs, hide=s['hide'])
        return [('depth', depth), ('depth, culled', culled), ('pixels', pix), ('probe', probe), ('mask', mask), ('normals', normals),
                ('rgba', rgba), ('depth of the colour pass', d2), ('face id', fid), ('skeleton', skel)]
    return GR.run_case(s, call, dict, _nothing, _side(),
                       claims=['rohm_depth_render', 'rohm_depth_probe', 'rohm_project_pixels', 'rohm_joint_occlusion_mask',
                               'rohm_vertex_normals', 'rohm_color_render', 'rohm_skeleton_mesh'])


@case('image[requantize, paste, overlay, flip]')
def _image():
    from rohm_amd import render
    s = GR.Slots(DEV)
    _two(s, 'img', lambda k: (seeded(7 + k, 2, 9, 11, 4).abs() * 120).clamp(0, 255).to(torch.uint8))
    _two(s, 'rgb', lambda k: (seeded(8 + 2 * k, 2, 9, 11, 3).abs() * 120).clamp(0, 255).to(torch.uint8))
    return GR.run_case(s, lambda s, h: [('requantize', render.requantize(s['img'], 0.5)), ('paste', render.paste(s['rgb'], s['img'])),
                                        ('overlay', render.overlay(s['rgb'], s['img'])), ('flip', render.flip_lr(s['img']))],
                       dict, _nothing, _side(),
                       claims=['rohm_image_requantize', 'rohm_image_paste', 'rohm_image_overlay', 'rohm_image_flip_lr'])


@case('train_helpers[cond, trajectory window in place]')
def _train_helpers():
    from rohm_amd.train import masks
    B, T = 3, 20
    words = lambda a: torch.from_numpy(np.asarray(a, np.uint32).view(np.int32).copy())
    s = GR.Slots(DEV)
    _two(s, 'src', lambda k: seeded(1 + 10 * k, B, T, 294))
    _two(s, 'clean', lambda k: seeded(2 + 10 * k, B, T, 294))
    s.add('joint bits', words([masks.joint_bits([1, 4, 7]), 0, masks.joint_bits(range(22))]),
          words([masks.joint_bits([0, 21]), masks.joint_bits(range(22)), 0]))
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    s.add('window', i32([[2, 9], [0, 0], [5, T]]), i32([[0, T], [3, 4], [0, 0]]))
    _two(s, 'vis bits', lambda k: words(np.random.Generator(np.random.PCG64(3 + k)).integers(0, 2 ** 22, size=(4, T))))
    s.add('vis index', torch.tensor([3, 0, 1]), torch.tensor([0, 2, 2]))         # rows of `vis bits`
    _two(s, 'traj', lambda k: seeded(4 + 10 * k, B, T, 13))
    s.add('traj window', i32([[0, 3], [7, 7], [10, T]]), i32([[5, T], [0, 1], [2, 2]]))

    def call(s, h):
        cond, clean_t = masks.train_cond(s['src'], s['clean'], joint_bits=s['joint bits'], window=s['window'], vis_bits=s['vis bits'],
                                         vis_index=s['vis index'], zero_contact=True)
        plain, _ = masks.train_cond(s['src'])
        return [('cond', cond), ('clean transposed', clean_t), ('cond, no masks', plain),
                ('trajectory window', masks.traj_window(s['traj'], s['traj window'], 9))]
    return GR.run_case(s, call, dict, _nothing, _side(), inplace=True, claims=['rohm_train_cond', 'rohm_train_traj_window'])


# ---- the data side and the metrics ----------------------------------------------------------------------------------------------------
@case('data[frames_to_world, clips, clips_repr, param noise, repr stats, batch, preprocess, keypoints, visibility]')
def _data():
    """The data-side entry points on one synthetic recording of 40 frames, clips of 16.  rohm_amass_preprocess is called through
    rohm_amd._lib (its wrapper uploads the recording index with a wait); rohm_keypoints_undistort is handed host arrays of the
    case's own, which are rewritten after the capture."""
    from rohm_amd import _lib
    from rohm_amd import preprocessing_amass as pa
    from rohm_amd.body_model import native_for
    from rohm_amd.data_loaders.clips import build_clips, clips_repr, undistort_keypoints, visibility_masks
    from rohm_amd.data_loaders.dataloader_amass import assemble, param_noise, repr_stats
    from rohm_amd.data_loaders.frames import frames_to_world
    from rohm_amd.utils import synth
    lib = _lib.lib()
    body = G._body().to(DEV)
    handle = native_for(body, DEV).handle
    mean, std = (torch.from_numpy(a).to(DEV) for a in synth.synthetic_stats(0))
    N, L = 40, 16
    s = GR.Slots(DEV)
    recs = [synth.synthetic_recording(3 + k, N, 'z') for k in (0, 1)]
    s.add('jw', *[torch.from_numpy(r[0]) for r in recs])
    s.add('world', *[torch.from_numpy(r[1]) for r in recs])
    s.add('starts', torch.tensor([0, 14, 24], dtype=torch.int32), torch.tensor([3, 10, 20], dtype=torch.int32))   # start + L <= N
    _two(s, 'joint noise', lambda k: seeded(5 + k, 3, L, 22, 3).double() * 0.01)
    for i, (key, d) in enumerate((('global_orient', 3), ('body_pose', 63), ('betas', 10), ('transl', 3))):
        _two(s, 'fit ' + key, lambda k, i=i, d=d: seeded(1 + i + 10 * k, 17, d) * 0.3)
    cam = np.eye(4, dtype=np.float32)
    cam[:3, :3], cam[:3, 3] = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]), (0.5, -0.25, 1.0)
    cam2 = cam.copy()
    cam2[:3, 3] += 0.25
    s.add('cam2world', torch.from_numpy(cam), torch.from_numpy(cam2))
    _two(s, 'p', lambda k: seeded(3 + 10 * k, 2, 5, 79).double() * 0.3)
    for i, (key, d, scale) in enumerate((('global_orient', 3, 1.0), ('transl', 3, 0.01), ('betas', 10, 0.1), ('body_pose', 63, 1.0))):
        _two(s, 'nz ' + key, lambda k, i=i, d=d, scale=scale: seeded(4 + i + 10 * k, 2, 5, d).double() * scale)
    _two(s, 'clean', lambda k: seeded(1 + 10 * k, 6, 15, 294))
    _two(s, 'noisy', lambda k: seeded(2 + 10 * k, 6, 15, 294))
    s.add('index', torch.tensor([4, 0, 5]), torch.tensor([1, 5, 2]))                    # items of the 6
    _two(s, 'rows', lambda k: seeded(2 + k, 7000, 294) * 2 + 0.5)
    for i, (key, d) in enumerate(pa.FRAME_KEYS):
        _two(s, 'amass ' + key, lambda k, i=i, d=d: seeded(10 + i + 20 * k, 17, d).double() * 0.3)
    _two(s, 'amass betas', lambda k: seeded(20 + k, 2, 10).double())
    s.add('rec of frame', (torch.arange(17) % 2).to(torch.int32), ((torch.arange(17) + 1) % 2).to(torch.int32))    # rows of the 2 betas
    _two(s, 'kp', lambda k: seeded(1 + 10 * k, N, 22, 3).abs() * torch.tensor([900.0, 500.0, 0.4]))
    _two(s, 'mask', lambda k: (seeded(2 + 10 * k, N, 25) > 0).float())
    pre_joints = torch.zeros(17, pa.NUM_JOINTS, 3, device=DEV)
    pre_params = torch.zeros(17, pa.PARAM_COLS, device=DEV)

    def host():
        return dict(K=np.array([[1060.53, 0.0, 951.30], [0.0, 1060.38, 536.77], [0.0, 0.0, 1.0]], np.float64),
                    k=np.array([0.052, -0.044, 0.0009, 0.0016, 0.003], np.float64))

    def rewrite(h):
        GR.rewrite_valid(h['K'], 0.0, 2000.0)
        GR.rewrite_valid(h['k'], -0.1, 0.1)

    def call(s, h):
        jw, world = frames_to_world(body, {k: s['fit ' + k] for k in ('global_orient', 'body_pose', 'betas', 'transl')}, s['cam2world'], device=DEV)
        out = [('joints_world', jw), ('smplx_world', world)]
        b = build_clips(s['jw'], s['world'], L, 2, 'z', None, stats=(mean, std), starts=s['starts'])
        b64 = build_clips(s['jw'], s['world'], L, 2, 'z', None, starts=s['starts'], params_f64=True)
        out += [('clips ' + k, v) for k, v in sorted(b.items())] + [('clips f64 ' + k, v) for k, v in sorted(b64.items())]
        idx = (s['starts'].long()[:, None] + torch.arange(L, device=DEV)[None]).reshape(-1)
        params = s['world'][idx].reshape(3, L, 79).clone()
        params[:, :, :6] = b64['orient_transl64']
        rep, joints = clips_repr(b64['cano_joints'].double(), params, stats=(mean, std), joint_noise=s['joint noise'], return_joints=True)
        out += [('repr', rep), ('joints', joints)]
        nz = {k: s['nz ' + k] for k in ('global_orient', 'transl', 'betas', 'body_pose')}
        out += [('param noise', param_noise(s['p'], nz)), ('param noise, additive', param_noise(s['p'], nz, additive=True))]
        m64, s64 = repr_stats(s['rows'])
        out += [('stats mean', m64), ('stats std', s64)]
        out += [('batch ' + k, v) for k, v in sorted(assemble(s['clean'], s['noisy'], s['index'], mean, std, overwrite_channels=22, cond='traj',
                                                              control=True).items())]
        _lib.check(lib.rohm_amass_preprocess(handle, *[_lib.ptr(s['amass ' + k]) for k, _ in pa.FRAME_KEYS], _lib.ptr(s['amass betas']),
                                             _lib.ptr(s['rec of frame']), 17, 2, _lib.ptr(pre_joints), _lib.ptr(pre_params),
                                             _lib.stream_ptr(DEV)), 'rohm_amass_preprocess')
        out += [('preprocessed joints', pre_joints), ('preprocessed params', pre_params)]
        jv, vv = visibility_masks(s['kp'], s['mask'], L, 2, starts=s['starts'])
        return out + [('undistorted', undistort_keypoints(s['kp'], h['K'], h['k'])), ('mask_joint_vis', jv), ('mask_vec_vis', vv)]
    return GR.run_case(s, call, host, rewrite, _side(),
                       claims=['rohm_smplx_frames_to_world', 'rohm_clips_build', 'rohm_clips_build_f64', 'rohm_clips_repr',
                               'rohm_smplx_param_noise', 'rohm_repr_stats', 'rohm_amass_batch', 'rohm_amass_preprocess',
                               'rohm_keypoints_undistort', 'rohm_visibility_masks'])


@case('metrics[amass, scene, result rows, traj report]')
def _metrics():
    """rohm_amass_metrics, rohm_scene_metrics and rohm_traj_report through rohm_amd._lib (their wrappers read the sums back, a wait,
    right after the launch); rohm_result_rows through its wrapper, whose item list the test cannot reach."""
    from rohm_amd import _lib
    from rohm_amd import evaluation as ev
    from rohm_amd.drivers import results as rs
    lib = _lib.lib()
    ptr, stream = _lib.ptr, _lib.stream_ptr
    n, T = 3, 20
    ds, _ = _stats_holder()
    s = GR.Slots(DEV)
    _two(s, 'jc', lambda k: seeded(1 + 10 * k, n, T, 22, 3))
    _two(s, 'jr', lambda k: seeded(1 + 10 * k, n, T, 22, 3) + 0.05 * seeded(2 + 10 * k, n, T, 22, 3))
    _two(s, 'rc', lambda k: seeded(3 + 10 * k, n, T, 294))
    _two(s, 'rr', lambda k: seeded(4 + 10 * k, n, T, 294))

    def scene_to_cano(k):
        m = torch.eye(4).repeat(n, 1, 1).contiguous()
        m[:, :3, 3] = 0.1 * k
        return m
    _two(s, 'tm', scene_to_cano)
    s.add('ground', torch.tensor([0.1, 0.0, -0.1]), torch.tensor([0.0, 0.2, 0.05]))
    _two(s, 'gt', lambda k: seeded(5 + 10 * k, n, T + 3, 22, 3))
    _two(s, 'vis', lambda k: (seeded(6 + 10 * k, n, T, 22) > 0).float())
    _two(s, 'x', lambda k: seeded(7 + 10 * k, n, 294, 1, T))
    _two(s, 'traj', lambda k: seeded(8 + 10 * k, n, T + 1, 22))
    f64 = dict(device=DEV, dtype=torch.float64)
    amass, scene, scene_ego = torch.zeros(n, 10, **f64), torch.zeros(n, ev._N_SCENE, **f64), torch.zeros(n, ev._N_SCENE, **f64)
    js = torch.zeros(n, T, 22, 3, device=DEV)
    report, elems = torch.zeros(n, rs._N_REPORT, **f64), torch.zeros(n, rs._N_REPORT, T, device=DEV)
    lower = sum(1 << j for j in ev.LOWER_JOINTS)

    def call(s, h):
        _lib.check(lib.rohm_amass_metrics(ptr(s['jc']), ptr(s['jr']), s['rc'].data_ptr() + 290 * 4, 294, s['rr'].data_ptr() + 290 * 4, 294,
                                          lower, 0, 0, n, T, ptr(amass), stream(DEV)), 'rohm_amass_metrics')
        _lib.check(lib.rohm_scene_metrics(ptr(s['jr']), ptr(s['tm']), ptr(s['ground']), ev.SCENE_UP_AXIS['prox'], None, 0, None, ptr(js), n, T,
                                          ptr(scene), stream(DEV)), 'rohm_scene_metrics')
        _lib.check(lib.rohm_scene_metrics(ptr(s['jr']), ptr(s['tm']), ptr(s['ground']), ev.SCENE_UP_AXIS['egobody'], ptr(s['gt']), T + 3,
                                          ptr(s['vis']), None, n, T, ptr(scene_ego), stream(DEV)), 'rohm_scene_metrics')
        rows = rs.result_rows([(s['x'], 'bc1t'), (s['rc'], 'btc', s['traj']), (s['rr'], 'btc'), (s['rc'], 'btc')], ds, T=T - 1)
        tracks = [s['jc'], s['jr'], s['jr'] * 1.01, s['jr'] * 0.99, s['jc'] + 0.01]
        _lib.check(lib.rohm_traj_report(*[ptr(j) for j in tracks], ptr(s['rc']), 294, ptr(s['rr']), 294, n, T, ptr(report), ptr(elems),
                                        stream(DEV)), 'rohm_traj_report')
        return ([('amass metrics', amass), ('scene metrics prox', scene), ('joints in the scene', js), ('scene metrics egobody', scene_ego)] +
                [(f'result rows {i}', r) for i, r in enumerate(rows)] + [('traj report', report), ('traj report terms', elems)])
    return GR.run_case(s, call, dict, _nothing, _side(),
                       claims=['rohm_amass_metrics', 'rohm_scene_metrics', 'rohm_result_rows', 'rohm_traj_report'])


# ---- tracks: quality, floor, fitting ---------------------------------------------------------------------------------------------------
@case('track[quality, floor clearance, candidates, moments, fit pose, shape moments]')
def _track():
    """rohm_track_quality through rohm_amd._lib (its wrapper reads the totals back right after the launch), the others through their
    wrappers with every operand on the device."""
    from rohm_amd import _lib, fit, floor, quality
    from rohm_amd.body_model import native_for
    from rohm_amd.utils import synth
    lib = _lib.lib()
    ptr = _lib.ptr
    nat = native_for(G._body().to(DEV), DEV)
    N, Nv, P, F = 24, 12, 300, 5
    s = GR.Slots(DEV)
    s.add('joints', *[torch.from_numpy(synth.synthetic_recording(3 + k, N, 'z')[0]) for k in (0, 1)])
    _two(s, 'kp', lambda k: seeded(1 + 10 * k, N, 22, 3).abs() * torch.tensor([900.0, 500.0, 0.4]))
    _two(s, 'ref', lambda k: torch.from_numpy(synth.synthetic_recording(3 + k, N, 'z')[0]) + 0.02 * seeded(2 + 10 * k, N, 22, 3))
    _two(s, 'ref mask', lambda k: (seeded(3 + 10 * k, N, 22) > 0).float())
    _two(s, 'gap', lambda k: (seeded(4 + 10 * k, N) > 0.5).to(torch.uint8))

    def scene2cam(k):
        m = torch.eye(4, dtype=torch.float64)
        m[:3, 3] = torch.tensor([0.1 * k, -0.2, 3.0], dtype=torch.float64)
        return m.reshape(16)
    _two(s, 'scene2cam', scene2cam)
    _two(s, 'verts', lambda k: seeded(5 + 10 * k, 2, 433, 3) * 0.5)
    s.add('times', torch.arange(N, dtype=torch.float64) / 30.0, torch.arange(N, dtype=torch.float64) / 25.0)
    s.add('valid', (torch.arange(Nv) * 2).to(torch.int32), (torch.arange(Nv) * 2 + 1).to(torch.int32))      # ascending, inside [0, N)
    _two(s, 'points', lambda k: seeded(6 + 10 * k, P, 3) * torch.tensor([2.0, 2.0, 0.02]))
    s.add('plane', torch.tensor([0.0, 0.0, 1.0, 0.0], dtype=torch.float64), torch.tensor([0.0, 0.6, 0.8, 0.01], dtype=torch.float64))
    s.add('origin', torch.zeros(3, dtype=torch.float64), torch.tensor([0.1, -0.1, 0.0], dtype=torch.float64))
    s.add('targets', *[torch.from_numpy(synth.synthetic_recording(5 + k, F, 'z')[0]) for k in (0, 1)])
    _two(s, 'conf', lambda k: seeded(7 + 10 * k, F, 22).abs().clamp(0, 1))
    _two(s, 'betas', lambda k: seeded(8 + 10 * k, F, 10) * 0.5)
    s.add('use', torch.tensor([1, 1, 0, 1, 1], dtype=torch.uint8), torch.tensor([0, 1, 1, 1, 0], dtype=torch.uint8))
    w_prior = torch.from_numpy(fit.default_w_prior()).to(DEV)
    rows = torch.zeros(N, len(quality.COLUMNS), device=DEV, dtype=torch.float64)
    totals = torch.zeros(2, quality.N_TOTALS, device=DEV, dtype=torch.float64)

    def call(s, h):
        _lib.check(lib.rohm_track_quality(ptr(s['joints']), N, 30.0, quality.UP_AXIS['z'], 1, 0.0, ptr(s['scene2cam']), 1060.53, 1060.38, 951.30,
                                          536.77, ptr(s['kp']), 0.2, ptr(s['ref']), ptr(s['ref mask']), ptr(s['gap']), ptr(rows), ptr(totals),
                                          _lib.stream_ptr(DEV)), 'rohm_track_quality')
        out = [('quality rows', rows), ('quality totals', totals), ('clearance', quality.floor_clearance(s['verts'], 'z', 0.0))]
        out += [('candidates', floor.floor_candidates(s['joints'], s['times'], s['valid'], keypoints=s['kp'])),
                ('moments', floor.floor_moments(s['points'], s['plane'], s['origin']))]
        params, report, normal = fit.fit_pose(nat, s['targets'], s['conf'], s['betas'], w_prior=w_prior, iters=4, want_normal=True)
        per_frame, moments = fit.shape_moments(nat, s['targets'], s['conf'], params, s['use'])
        return out + [('fit params', params), ('fit report', report), ('fit normal', normal), ('shape moments per frame', per_frame),
                      ('shape moments', moments)]
    return GR.run_case(s, call, dict, _nothing, _side(),
                       claims=['rohm_track_quality', 'rohm_floor_clearance', 'rohm_floor_candidates', 'rohm_floor_moments', 'rohm_fit_pose',
                               'rohm_fit_shape_moments'])


# ---- the headers next to rohm_hip.h ----------------------------------------------------------------------------------------------------
def _header_case(header, inputs, call):
    """The case of tests/header_cases.py: value sets 7 and 8 in the slots; every stream-taking function of the header, and nothing
    else, is recorded."""
    s = GR.Slots(DEV)
    for k in inputs(7):
        s.add(k, torch.from_numpy(np.array(inputs(7)[k])), torch.from_numpy(np.array(inputs(8)[k])))
    claims = set(SO.abi_stream_functions(SM.abi_headers()[header]))
    r = GR.run_case(s, lambda s, h: call({k: s[k] for k in inputs(7)}), dict, _nothing, _side(), claims=claims)
    assert r['replays'] >= 3 and r['log'].recorded() == claims
    return r


for _name, _case in HC.CASES.items():
    case(_name)(lambda c=_case: _header_case(*c))


# ================================================================================================ the tests
@pytest.mark.parametrize('name', sorted(CASES))
def test_a_replay_does_what_the_recorded_call_would_do_again(name):
    r = _result(name)
    if isinstance(r, BaseException):
        raise r
    nodes, edges, forks = r['shape']
    print(f'{name}: {len(r["log"].capturing)} recorded calls of {sorted(r["log"].recorded())}, {nodes} nodes, {edges} edges, {forks} forks, '
          f'capture {r["record_seconds"]:.3f} s, instantiate {r["instantiate_seconds"]:.3f} s, case {r["seconds"]:.3f} s')
    assert nodes > 0 and edges >= nodes - 1


def test_the_control_stream_and_the_one_stream_order_replay_the_same_bits():
    a = _result('trajnet[loop, TrajControl, control stream, 4 steps]')
    b = _result('trajnet[loop, TrajControl, one stream, 4 steps]')
    for r in (a, b):
        if isinstance(r, BaseException):
            raise r
    assert a['final'] and not SM.differences(a['final'], b['final'])
    # ... and they are two DIFFERENT graphs: the one-stream capture is a chain; with the control stream the graph forks (the caller's
    # stream hands the time table, and from step 2 on the "consumed" events, to the branch) and holds more edges than a chain
    (na, ea, fa), (nb, eb, fb) = a['shape'], b['shape']
    print(f'control stream: {na} nodes, {ea} edges, {fa} forks; one stream: {nb} nodes, {eb} edges, {fb} forks')
    assert fb == 0 and eb == nb - 1, (nb, eb, fb)
    assert fa >= 1 and ea > na - 1, (na, ea, fa)


def test_every_replayed_entry_point_was_called_while_recording():
    """Over all cases: the call logs hold graph_replay.REPLAYED to the truth, family by family."""
    results = {name: _result(name) for name in sorted(CASES)}
    recorded = {}
    for name, r in results.items():
        if not isinstance(r, BaseException):
            recorded.setdefault(G.family(name), set()).update(r['log'].recorded())
    missing = {f: fam for f, fam in GR.REPLAYED.items() if f not in recorded.get(fam, set())}
    assert not missing, f'REPLAYED names entry points that no case of their family called while recording: {missing}'
    extra = set().union(*recorded.values()) - set(GR.REPLAYED) if recorded else set()
    assert not extra, f'recorded but not in REPLAYED: {sorted(extra)}'
    ok = [r for r in results.values() if not isinstance(r, BaseException)]
    slow = max(ok, key=lambda r: r['seconds'])
    print('cases:', len(results), 'graphs:', len(ok), 'replays:', sum(r['replays'] for r in ok),
          'seconds in all:', round(sum(r['seconds'] for r in ok), 2), 'slowest:', [n for n, r in results.items() if r is slow],
          round(slow['seconds'], 2), 'nodes in all:', sum(r['shape'][0] for r in ok))
    big = results['trajnet[loop, TrajNet, 130 steps]']
    assert not isinstance(big, BaseException) and big['shape'][2] == 0          # one stream: a chain
    print(f'130-step TrajNet graph: {big["shape"][0]} nodes, capture {big["record_seconds"]:.3f} s, instantiate {big["instantiate_seconds"]:.3f} s')


# ================================================================================================ the Python layer
def test_adamw_step_raises_while_recording_and_names_the_frozen_step():
    from rohm_amd import optim
    ps = [seeded(i, *shape).to(DEV).requires_grad_() for i, shape in enumerate([(5,), (300, 7)])]
    opt = optim.AdamW(ps, lr=1e-2, max_grad_norm=1.0)
    for q in ps:
        q.grad = torch.ones_like(q)
    side = _side()
    with torch.cuda.stream(side):
        opt.step()                                                  # step 1, eagerly
    before = [q.detach().clone() for q in ps]
    flag, graph = torch.zeros(4, device=DEV), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        flag.fill_(7.0)
        with pytest.raises(RuntimeError, match='frozen step count 2'):
            opt.step()
    graph.replay()                                                  # nothing was issued: the capture survived and holds the marker only
    torch.cuda.synchronize()
    assert flag.tolist() == [7.0] * 4
    assert all(torch.equal(a, b.detach()) for a, b in zip(before, ps))
    assert all(float(opt.state[q]['step']) == 1.0 for q in ps)     # the counters did not move
    with torch.cuda.stream(side):
        opt.step()
    torch.cuda.synchronize()
    assert all(float(opt.state[q]['step']) == 2.0 for q in ps)
    # the very FIRST step of an optimiser under a capture: refused before the closure runs and before any state is created
    fresh, ran = optim.AdamW(ps, lr=1e-2), []
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        flag.fill_(9.0)
        with pytest.raises(RuntimeError, match='frozen step count 1'):
            fresh.step(lambda: ran.append(1))
    graph.replay()
    torch.cuda.synchronize()
    assert flag.tolist() == [9.0] * 4 and not ran and len(fresh.state) == 0


def test_posenet_forward_with_dropout_raises_while_recording():
    """Train mode, dropout > 0: the seed is drawn on the host, a graph would repeat the masks.  (Dropout 0 records: the train cases.)"""
    net = G._make_posenet(None, L=1, dropout=0.1).train()
    B, T = 2, 16
    x, c = seeded(1, B, 294, 1, T).to(DEV), seeded(2, B, 294, 1, T).to(DEV)
    t = torch.tensor([1, 38], device=DEV)
    side = _side()
    with torch.cuda.stream(side):
        net({'x_t': x, 'cond': c}, t)                               # eagerly it draws a seed and runs
    flag, graph = torch.zeros(4, device=DEV), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        flag.fill_(7.0)
        with pytest.raises(RuntimeError, match='dropout seed is drawn on the host'):
            net({'x_t': x, 'cond': c}, t)
    graph.replay()
    torch.cuda.synchronize()
    assert flag.tolist() == [7.0] * 4
