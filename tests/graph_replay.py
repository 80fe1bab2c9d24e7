"""TEST INFRASTRUCTURE ONLY (host side of tests/test_gpu_graph_replay.py): static input slots, the rewrite of host arrays with other
VALID values, a call log that notes whether each call was made while its stream was recording, the record / replay protocol, and
the three tables that say what becomes of every stream-taking entry point of the public headers under a graph capture.  Nothing in
rohm_amd/ imports this module; it has no GPU code of its own.

include/rohm_hip.h ("Conventions", recordable calls) promises that a call on a recording stream replays as the same call made again
with the same argument values: device operands are read at replay time, host scalars and host arrays at the call.  An eager test
cannot see a breach: a recorded copy from a caller's host array, a decision taken once on the host, a first-call clear that is not
a node -- each gives the right answer the first time.  The protocol (`run_case`):

  1. eager, on a side stream, after one warm-up call: E1 = the call on value set 1, E2 = on value set 2 (another seed; integer inputs
     get other VALID values); for in-place operands also E11 = two calls in a row on set 1;
  2. record on set 1 under `stale_memory.poison(all-ones)` -- every torch.empty a wrapper makes while recording is filled by a
     RECORDED fill, so each replay meets poisoned outputs and workspaces of its own -- then rewrite every host array the call was given
     (`rewrite_valid`, `rewrite_tables`) and drop it;
  3. replay, compare with E1;
  4. poison the outputs and the buffers the case names (workspaces cached by a handle: allocated by the warm-up, so no recorded fill
     covers them), copy set 2 into the slots, replay, compare with E2;
  5. poison, copy set 1 back, replay, compare with E1; in-place cases replay twice without a wait in between and compare with E11;
  6. the call log shows every function the case claims was called while the stream was recording, and none outside a recording;
  7. the exchange status the case owns is clean.

Every device input lives in a `Slots` slot and receives its values by a device-to-device copy on the replay stream, so the recorded
addresses stay put.  The two "state by purpose" items of the header are treated as tests/stale_memory.py treats them: a training
step records forward and backward in ONE graph (the `saved` buffer never crosses a replay), and an armed exchange header is
poisoned like anything else (the recorded arm kernels find no magic word and arm it again)."""
import contextlib

import numpy as np
import torch

import stale_memory as SM
import stream_order as SO

ONES = SM.PATTERNS['ones']


# ---- the three tables ----------------------------------------------------------------------------------------------------------
# entry point -> the case family of tests/test_gpu_graph_replay.py that records it (the call log holds the table to the truth)
REPLAYED = {
    'rohm_gemm_f32': 'ops', 'rohm_gemm_res_layernorm_f32': 'ops', 'rohm_output_process_f32': 'ops', 'rohm_layernorm_f32': 'ops',
    'rohm_attention_f32': 'ops',
    'rohm_planes_split': 'planes', 'rohm_gemm_planes': 'planes', 'rohm_gemm_planes_ln': 'planes', 'rohm_layernorm_planes_f32': 'planes',
    'rohm_attention_planes_f32': 'planes',
    'rohm_ddpm_step': 'ddpm', 'rohm_ddpm_step_table': 'ddpm', 'rohm_posenet_dropout_mask': 'ddpm', 'rohm_q_sample': 'ddpm',
    'rohm_posenet_forward': 'posenet', 'rohm_posenet_sample_loop': 'posenet',
    'rohm_trajnet_forward': 'trajnet', 'rohm_trajnet_sample_loop': 'trajnet',
    'rohm_posenet_train_forward': 'train', 'rohm_posenet_train_backward': 'train', 'rohm_trajnet_train_forward': 'train',
    'rohm_trajnet_train_backward': 'train', 'rohm_grad_norm': 'train', 'rohm_adamw_step': 'train',
    'rohm_guidance_skating_grad': 'guided', 'rohm_guidance_skating_prepare': 'guided', 'rohm_guidance_skating_apply': 'guided',
    'rohm_guidance_proj2d_grad': 'guided',
    'rohm_smplx_forward': 'smplx', 'rohm_smplx_joints': 'smplx',
    'rohm_repr_joints': 'repr', 'rohm_repr_joints_vjp': 'repr', 'rohm_traj_rederive': 'repr',
    'rohm_export_smplx': 'export', 'rohm_export_smplx_blend': 'export',
    'rohm_depth_render': 'render', 'rohm_depth_probe': 'render', 'rohm_project_pixels': 'render', 'rohm_joint_occlusion_mask': 'render',
    'rohm_vertex_normals': 'render', 'rohm_color_render': 'render', 'rohm_skeleton_mesh': 'render',
    'rohm_image_requantize': 'image', 'rohm_image_paste': 'image', 'rohm_image_overlay': 'image', 'rohm_image_flip_lr': 'image',
    'rohm_train_cond': 'train_helpers', 'rohm_train_traj_window': 'train_helpers',
    'rohm_smplx_frames_to_world': 'data', 'rohm_clips_build': 'data', 'rohm_clips_build_f64': 'data', 'rohm_clips_repr': 'data',
    'rohm_smplx_param_noise': 'data', 'rohm_repr_stats': 'data', 'rohm_amass_batch': 'data', 'rohm_amass_preprocess': 'data',
    'rohm_keypoints_undistort': 'data', 'rohm_visibility_masks': 'data',
    'rohm_amass_metrics': 'metrics', 'rohm_scene_metrics': 'metrics', 'rohm_result_rows': 'metrics', 'rohm_traj_report': 'metrics',
    'rohm_track_quality': 'track', 'rohm_floor_clearance': 'track', 'rohm_floor_candidates': 'track', 'rohm_floor_moments': 'track',
    'rohm_fit_pose': 'track', 'rohm_fit_shape_moments': 'track',
    'rohm_mv_triangulate': 'multiview', 'rohm_mv_residuals': 'multiview',
    'rohm_fit_views_pose': 'fit_views',
    'rohm_rig_pair_hypotheses': 'rig', 'rohm_rig_pair_moments': 'rig', 'rohm_rig_ba_moments': 'rig', 'rohm_rig_ba_update': 'rig',
}

# entry point -> the header sentence that says it waits (looked up in stream_order.header_prose by the host test)
REFUSED_WHILE_RECORDING = {
    'rohm_track_resample': 'rohm_track_resample waits for its stream to check valid_idx on the host and is refused on a recording stream.',
    'rohm_floor_hypotheses': 'rohm_floor_hypotheses waits for its stream to check the triples on the host and is refused on a recording '
                             'stream.',
    'rohm_posenet_exchange_status': 'rohm_posenet_exchange_status waits for its stream to read the status word and is refused on a '
                                    'recording stream.',
}

# entry point -> why no case can record it (none today: a new entry needs a sentence in the pull request that adds it)
EXEMPT = {}


def partition_errors(stream_functions=None):
    """What keeps the three tables from partitioning the header's stream-taking functions: dict(missing, unknown, twice)."""
    names = set(SO.abi_stream_functions() if stream_functions is None else stream_functions)
    tables = [set(REPLAYED), set(REFUSED_WHILE_RECORDING), set(EXEMPT)]
    listed = set().union(*tables)
    twice = {n for n in listed if sum(n in t for t in tables) > 1}
    return dict(missing=sorted(names - listed), unknown=sorted(listed - names), twice=sorted(twice))


# ---- input slots ---------------------------------------------------------------------------------------------------------------
class Slots:
    """Static device memory for the inputs of a case: `add(name, set 1, set 2)` stages both value sets on the device and allocates the
    slot; `load(k)` copies value set k (1 or 2) into every slot, device to device, on the current stream.  A value set of another
    shape or dtype than the first is refused: the recorded addresses and sizes are the first set's."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.slot, self.values = {}, {}

    def add(self, name, *value_sets):
        if name in self.slot:
            raise ValueError(f'slot {name!r} exists')
        if len(value_sets) != 2:
            raise ValueError(f'slot {name!r} needs two value sets, got {len(value_sets)}')
        first = value_sets[0]
        for k, v in enumerate(value_sets[1:], 2):
            if tuple(v.shape) != tuple(first.shape) or v.dtype != first.dtype:
                raise ValueError(f'slot {name!r}: value set {k} is {tuple(v.shape)} {v.dtype}, value set 1 is {tuple(first.shape)} {first.dtype}')
        self.values[name] = [v.detach().to(self.device).contiguous().clone() for v in value_sets]
        self.slot[name] = SM.fill_bytes(SM._REAL_EMPTY(first.shape, dtype=first.dtype, device=self.device), SO.prefill_word(first.dtype))
        return self.slot[name]

    def __getitem__(self, name):
        return self.slot[name]

    def load(self, k):
        if k not in (1, 2):
            raise ValueError(f'value set {k}: there are two')
        for name, slot in self.slot.items():
            slot.copy_(self.values[name][k - 1], non_blocking=True)


# ---- host arrays: other VALID values of the same type --------------------------------------------------------------------------
def rewrite_valid(a, lo=None, hi=None):
    """Overwrite the numpy array `a` IN PLACE with other values of the same dtype and shape inside [lo, hi] (default: the array's own
    minimum and maximum): every element is mirrored (lo + hi - x) and the order reversed; where that leaves an element as it was
    (a constant array, a symmetric one) it takes the range's other end or its neighbour's value instead.  Raises where the range
    holds one value only: a stale read could not show.  -> the array's former contents (a copy)."""
    if not isinstance(a, np.ndarray) or not a.flags.writeable or not a.flags.c_contiguous:
        raise ValueError('rewrite_valid takes a writeable C-contiguous numpy array')
    old = a.copy()
    if a.size == 0:
        return old
    lo = old.min() if lo is None else a.dtype.type(lo)
    hi = old.max() if hi is None else a.dtype.type(hi)
    if not (lo <= old.min() and old.max() <= hi):
        raise ValueError(f'the array leaves [{lo}, {hi}]')
    if lo == hi:
        raise ValueError(f'every valid value is {lo}: a rewrite cannot differ (give lo / hi)')
    flat, was = a.reshape(-1), old.reshape(-1)
    flat[:] = (lo + (hi - was))[::-1]
    same = flat == was
    flat[same] = np.where(was[same] == lo, hi, lo)
    assert a.dtype == old.dtype and a.shape == old.shape and lo <= a.min() and a.max() <= hi and not (a == old).any()
    return old


def rewrite_tables(pointer_tables, numel_table):
    """Overwrite ctypes pointer tables (arrays of c_void_p, one entry per tensor) and their table of element counts in place so that
    ANY mix of old and new entries stays inside a buffer: every pointer becomes the table's pointer of the LARGEST tensor and every
    count the SMALLEST count.  A stale read then updates the wrong tensor, or too little of it: a wrong result, never a wild access."""
    counts = list(numel_table)
    if len(counts) < 2:
        raise ValueError('a table of fewer than two tensors cannot be rewritten to differ')
    big = counts.index(max(counts))
    for table in pointer_tables:
        if len(table) != len(counts):
            raise ValueError('pointer and count tables differ in length')
        keep = table[big]
        for i in range(len(counts)):
            table[i] = keep
    for i in range(len(counts)):
        numel_table[i] = min(counts)


# ---- the call log, with the recording state ------------------------------------------------------------------------------------
def _capturing():
    return bool(torch.cuda.is_current_stream_capturing())


class RecordingLog(SO.CallLog):
    """stream_order.CallLog (every call is held to the current stream, by name) that also notes, per call, whether the current stream
    was recording a graph: `capturing` holds (function, bool)."""

    def __init__(self, is_capturing=_capturing, **kw):
        super().__init__(**kw)
        self.is_capturing, self.capturing = is_capturing, []

    def _wrap(self, name, real, at):
        inner = super()._wrap(name, real, at)

        def logged(*args):
            self.capturing.append((name, bool(self.is_capturing())))
            return inner(*args)
        logged.__wrapped__ = real
        return logged

    def recorded(self):
        return {name for name, cap in self.capturing if cap}

    def outside(self):
        return sorted({name for name, cap in self.capturing if not cap})

    def check_claims(self, claims):
        """Check 6: every claimed function was called while recording, and nothing was called outside a recording."""
        missing = sorted(set(claims) - self.recorded())
        assert not missing, f'never called while the stream was recording: {missing}'
        assert not self.outside(), f'called while the stream was NOT recording: {self.outside()}'


def record(fn, stream, lib_obj=None, stream_at=None, poison=True):
    """Record `fn()` into a torch.cuda.CUDAGraph on `stream` under the call log (and all-ones poison of what it allocates).  The
    graph is kept (`keep_graph=True`: `raw_cuda_graph()` stays valid for a look at its nodes and edges) and instantiated here, by
    itself, so that the time of the instantiation is known apart from the capture's.
    -> (graph, what fn returned, the log, seconds of the instantiation)"""
    import time
    if lib_obj is None:
        from rohm_amd import _lib
        lib_obj = _lib.lib()
    stream_at = SO.abi_stream_functions() if stream_at is None else stream_at
    log = RecordingLog()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with log.installed(lib_obj, stream_at), (SM.poison(ONES) if poison else contextlib.nullcontext()):
        with torch.cuda.graph(graph, stream=stream):
            out = fn()
    t0 = time.perf_counter()
    graph.instantiate()
    return graph, out, log, time.perf_counter() - t0


# ---- the protocol --------------------------------------------------------------------------------------------------------------
def poison_tensors(tensors):
    for t in tensors:
        SM.fill_bytes(t, ONES)


def run_case(slots, call, host, rewrite, side, claims, inplace=False, buffers=lambda: (), status=None, lib_obj=None, stream_at=None,
             eager_env=None, after_record=None):
    """The protocol of the module docstring.
      slots    Slots with both value sets of every device input
      call     call(slots, h) -> [(label, tensor)]: the entry point(s), with the host arrays `h`
      host     host() -> a fresh set of host arrays (any object `call` understands)
      rewrite  rewrite(h): overwrite every host array of `h` with other valid values (after the capture; `h` is dropped afterwards)
      buffers  buffers() -> device tensors besides the outputs to poison between replays (workspaces a handle caches)
      status   status(): raises unless the exchange status the case owns is clean (check 7)
      eager_env     environment variables for the eager calls only (a form the recorded call must take by itself)
      after_record  after_record(): checks on the process-wide read-outs of the recording call
    -> dict(graph, log, seconds, record_seconds (the capture), instantiate_seconds, final, out, replays) after all seven checks passed; `final` is the last replay on set 1."""
    import time
    t0 = time.perf_counter()
    with torch.cuda.stream(side), SM.env(**(eager_env or {})):
        slots.load(1)
        call(slots, host())                                      # the warm-up (caches, lazily created streams, first-call probes)
        slots.load(1)
        e1 = SM.snapshot(call(slots, host()))
        slots.load(2)
        e2 = SM.snapshot(call(slots, host()))
        e11 = None
        if inplace:
            slots.load(1)
            call(slots, host())
            e11 = SM.snapshot(call(slots, host()))
        side.synchronize()
        assert SM.differences(e1, e2), 'the two value sets give the same outputs: the case could not tell a stale input'
        slots.load(1)
    side.synchronize()
    h = host()
    t1 = time.perf_counter()
    graph, out, log, instantiate_seconds = record(lambda: call(slots, h), side, lib_obj, stream_at)
    record_seconds = time.perf_counter() - t1 - instantiate_seconds
    if after_record is not None:
        after_record()
    rewrite(h)
    del h
    final, replays = [], [1]
    with torch.cuda.stream(side):
        def replay_and_compare(k, want, what, times=1):
            replays[0] += times
            poison_tensors([t for _, t in out] + list(buffers()))
            slots.load(k)
            for _ in range(times):
                graph.replay()
            got = SM.snapshot(out)
            side.synchronize()
            diff = SM.differences(got, want)
            assert not diff, f'{what}: the replay differs from the eager call: {diff[:3]} (output, (first differing element, replay, eager))'
            return got
        slots.load(1)
        graph.replay()                                           # check 3: nothing poisoned yet beyond what the graph itself fills
        got = SM.snapshot(out)
        side.synchronize()
        diff = SM.differences(got, e1)
        assert not diff, f'first replay: differs from the eager call on set 1: {diff[:3]}'
        replay_and_compare(2, e2, 'replay on value set 2')
        final = replay_and_compare(1, e1, 'replay on value set 1 again')
        if inplace:
            replay_and_compare(1, e11, 'two replays in a row', times=2)
    log.check_claims(claims)
    if status is not None:
        status()
    return dict(graph=graph, log=log, seconds=time.perf_counter() - t0, record_seconds=record_seconds, instantiate_seconds=instantiate_seconds,
                final=final, out=out,
                replays=replays[0])
