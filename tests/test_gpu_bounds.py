"""GPU: no entry point reads or writes outside the operands it is given, and of a workspace it uses no more than its `*_bytes`
function says (include/rohm_hip.h, "Conventions").

tests/test_gpu_stale_memory.py poisons what a buffer HOLDS; tightly sized tensors still hide an access one row past a buffer (it
lands in the caching allocator's rounding or in a neighbour and reads finite leftovers).  Here every case of that module's registry
(imported, not copied: `G.CASES`, `G._run`, `stale_memory.differences`) and the cases of EXTRA below run once more

  (a) under `guarded_memory.guard()`: every output, workspace, scratch and saved buffer the wrappers allocate lies between two 1 MiB
      bands of 0xFF.  No band byte may change, nothing may be allocated past the guard without a named reason, and the outputs equal
      the run in plain zero-filled memory BIT FOR BIT (a load from a band is NaN and would show).  Rule (b) of the stale-memory
      module (a case whose two plain runs differ uses its ORACLE entry) applies unchanged; no case needs it.
  (b) with the allocator's log held against the library's own byte counts: every value a `rohm_*_bytes` function returned during the
      guarded run is the exact size of an allocation (or, for a cached workspace, not larger than one that is).  The two wrappers that
      ask for MORE than the library says (ops.gemm_res_layernorm: +16 ints, ops.output_process: +64 ints, for their own alignment) are
      driven directly through `_lib` with a scratch of exactly `*_scratch_bytes` from the guarded allocator.
  (c) with every input that passes through the registry's `_d` placed on a canvas (`guarded_memory.place(t, 'aligned')`): outputs
      equal (a)'s baseline bit for bit and every canvas is untouched afterwards, except the operands a call updates in place
      (INPLACE below).  For the two training families every parameter's `.data` sits on a canvas of its own as well: the library
      reads the live parameters in place.
  (d) with x_t, cond, noise, the guidance inputs and d_out as BATCH SLICES (`place(t, 'slice')`: 8 bytes past a 16-byte boundary):
      results equal the aligned run bit for bit.  For posenet_train every parameter is, besides, a view one float into a flat buffer
      (4 bytes past a 512-byte boundary: the 4-byte path of the LayerNorm kernels' gamma / beta loads).  Read before run: every
      kernel behind these entry points reads the caller's [B, 294, 1, T] tensors with 4-byte accesses (pack_kernel, finish_kernel,
      finish_pack_kernel, the output heads, ddpm_step*, the training tile loads, traj_copy) or, in the stack form's closing phase,
      with 16-byte accesses declared 4-byte aligned (rows of T = 143 floats are never 16-byte aligned, slice or not), and reads the
      training parameters with 4-byte accesses.  The one exception was fixed here (Findings).
  (d') for the three headers next to rohm_hip.h (multiview, fit_views, rig), whose opening comments promise that an operand "needs
      the alignment of its element only": every input on an 'offset' canvas and every allocation from `guard(offset=True)`, so that
      inputs, outputs and workspaces all start ONE ELEMENT past a 512-byte boundary (4 bytes for float32 / int32, 8 for float64 /
      int64); results equal the aligned run bit for bit, canvases and bands untouched.  A further test counts, through the loaded
      library, that each of these three cases calls every declaration of its header, the host-only ones included.
  (e) once with a planted overrun, to show the check can fail: `rohm_ddpm_step` with n four floats larger than its tensors, inputs on
      canvases, the output from the guarded allocator.  Every access stays inside the test's own allocations.

Inputs that do NOT pass through `_d` and so stay tightly sized in (c) / (d) -- nobody should take them for covered:
  * index tensors made with torch.tensor(..., device=DEV): the timesteps of posenet_* / trajnet_* / ddpm / train_helpers (q_sample),
    export_smplx's frame_clip / frame_t, amass's item index, clips_repr's idx;
  * what wrappers build from numpy arrays or host lists: the loops' coef / t_model tables, track_resample (all inputs), depth / color
    (faces, camera, adjacency, templates: render.icosphere / cylinder), keypoints' camera matrix, train_helpers' joint_bits / window /
    vis_bits, track_quality's scene2cam, amass preprocessing's rec_of_frame, the optimiser's moment buffers (torch.zeros_like);
  * tensors a case derives on the device (.contiguous(), .clone(), .double(), torch.cat, permute): clips_repr's params / joints,
    repr's xb, amass's noisy[:3], metrics' jr, everything a model computes between two entry points (posenet_guided's pred_xstart);
  * the weights of the inference handles (copied at create); cond of repr (torch.empty + copy_: an allocation, covered by (a)).

In-place operands exempt from `untouched()` (their bands are still checked): planes: `layernorm` (layernorm_planes_ normalises x in
place); posenet_loop and trajnet_loop: `x`; train_helpers: `trajectory window` (rohm_train_traj_window); optim: the four parameters
(canvases #0 .. #3).  `layernorm[144x512]`'s x is an allocation (torch.empty), covered by (a).

Findings:
  * csrc/posenet_train.hip, ln_fwd_kernel / ln_bwd_kernel: gamma and beta were read from the caller's LIVE parameter pointers with
    16-byte loads although the header promises nothing about their alignment (a parameter that is a view into a flat buffer at an odd
    multiple of 4 bytes would have faulted).  Found by reading, before any misaligned run; fixed with a 4-byte path taken when the
    address is not 16-byte aligned (param4).  The gradient stores of ln_bwd_kernel (ds, gx, dd) go to the 16-byte-aligned `scratch`,
    not to the caller's `grads`: those are written by colsum / slab_sum with 4-byte stores.
  * Method: arithmetic hands a quiet NaN on with its bits, so a store of what was LOADED from an all-ones band into an all-ones band
    changes nothing.  Measured on MI355X with (e)'s call: with all-ones input bands the four words behind the output read 0xFFFFFFFF
    and violations() is empty; with the NaN 0x7FC00001 they read 0x7FC00001 and the overrun is reported at offset 504504.  (e)
    therefore gives its input canvases that other NaN; (a) and (c) are separate runs, so there a band's NaN shows in the outputs
    instead.  What stays unseen: a store BEHIND a guarded buffer of a value loaded from another guarded buffer's band.
  * Nothing else: on MI355X no case writes a band byte, changes its result between bands or changes an input, no allocation passes
    the guard, and every `rohm_*_bytes` value is the exact size its wrapper asks for but for the two named under (b).  Held to their
    number by this module: rohm_gemm_res_layernorm_scratch_bytes, rohm_output_process_scratch_bytes, rohm_planes_bytes,
    rohm_posenet_workspace_bytes, rohm_posenet_train_saved_bytes / _scratch_bytes, rohm_trajnet_workspace_bytes,
    rohm_trajnet_train_saved_bytes / _scratch_bytes, rohm_guidance_workspace_bytes, rohm_smplx_lbs_workspace_bytes,
    rohm_repr_stats_scratch_bytes, rohm_depth_workspace_bytes, rohm_color_workspace_bytes, rohm_grad_norm_scratch_bytes
    (rohm_clips_scratch_bytes is 0 at these clip lengths: nothing to hold; rohm_posenet_stack_timeline_bytes is not run).

Sizes (MI355X): 86 cases (81 of the registry, 5 here), 352 guarded allocations in (a), 1170 canvases in (c); per family, cases /
guarded allocations / canvases: amass 1 / 15 / 16, attention 2 / 2 / 2, clips_build 2 / 10 / 4, clips_build_f64 1 / 6 / 2, clips_repr
1 / 9 / 3, color 1 / 8 / 4, ddpm 1 / 4 / 5, depth 1 / 7 / 2, export_smplx 1 / 3 / 3, export_smplx_blend 1 / 4 / 3, fit 1 / 7 / 14, fit_views 1 / 6 / 6,
floor 1 / 8 / 19, gemm 1 / 2 / 7, gemm_res_layernorm 2 / 8 / 12, guidance_proj2d 1 / 2 / 5, guidance_skating 1 / 3 / 1,
guidance_skating_split 1 / 3 / 1, keypoints 1 / 3 / 3, layernorm 1 / 1 / 2, metrics 1 / 11 / 8, multiview 1 / 10 / 4, optim 1 / 2 / 12, output_process
2 / 6 / 12, planes 2 / 16 / 19, posenet_forward 9 / 18 / 18, posenet_guided 1 / 6 / 3, posenet_loop 3 / 9 / 9, posenet_train
4 / 24 / 100 (22 of every 25 are parameters), repr 1 / 11 / 5, repr_stats 1 / 6 / 2, rig 1 / 12 / 7, smplx_forward 8 / 20 / 24, smplx_joints 1 / 2 / 4,
track_quality 1 / 5 / 7, track_resample 1 / 8 / 0, train_helpers 1 / 7 / 7, trajnet_forward 7 / 14 / 21, trajnet_loop 14 / 42 / 56,
trajnet_train 3 / 12 / 738 (186 / 270 / 270 parameters).  In (d') 4 / 6 / 7 inputs and 10 / 6 / 12 allocations (multiview / fit_views
/ rig) sit one element past a boundary; rohm_rig_pair_ws_bytes (4224) and rohm_rig_ba_ws_bytes (20000) are held to their number as
well.  Wall time of the whole module, 182 tests: 21 s as measured run alone (the slowest test 1.4 s); with the three header cases,
194 tests, 16.6 s summed over its tests when run after tests/test_gpu_stale_memory.py in one process (the slowest 0.72 s; each of
the twelve tests of the three header cases below 5 ms).  Every case runs four times (two plain runs, one guarded, one on
canvases), the eleven of (d) and the three of (d') a fifth time, those three a sixth time for the count of their calls."""
import contextlib

import numpy as np
import pytest
import torch

import guarded_memory as GM
import header_cases as HC
import stale_memory as SM
import test_gpu_stale_memory as G
from helpers import seeded

pytestmark = pytest.mark.gpu
DEV = G.DEV

# ================================================================================================ entry points the registry does not reach
EXTRA = {}              # name -> callable returning [(label, tensor), ...], inputs through G._d (as the registry's cases)
EXTRA_COVERAGE = {      # family -> the entry points its cases run
    'gemm': ['rohm_gemm_f32'],
    'track_quality': ['rohm_track_quality', 'rohm_floor_clearance'],
    'floor': ['rohm_floor_candidates', 'rohm_floor_hypotheses', 'rohm_floor_moments'],
    'fit': ['rohm_fit_pose', 'rohm_fit_shape_moments'],
    'export_smplx_blend': ['rohm_export_smplx_blend'],
}


def xcase(name):
    def deco(fn):
        assert name not in EXTRA and name not in G.CASES
        EXTRA[name] = fn
        return fn
    return deco


def _np(a):
    return G._d(torch.from_numpy(np.array(a)))


@xcase('gemm[150x100x64, bias + residual and GELU]')
def _gemm():
    from rohm_amd import ops
    M, N, K = 150, 100, 64                                      # ragged in M and N: part-filled tiles on both edges
    a, w, bias, res = seeded(1, M, K), seeded(2, N, K) / 8.0, seeded(3, N), seeded(4, M, N)
    return [('bias + residual', ops.gemm(G._d(a), G._d(w), G._d(bias), G._d(res), epi=ops.EPI_BIAS_RES)),
            ('gelu', ops.gemm(G._d(a), G._d(w), G._d(bias), epi=ops.EPI_BIAS_GELU))]


@xcase('track_quality[N50, camera, reference, gaps; clearance V7]')
def _track_quality():
    import test_gpu_quality as TQ
    from rohm_amd.quality import floor_clearance, track_quality
    d = TQ.make_inputs(50, 7)
    q = track_quality(_np(d['joints']), 30.0, 'z', TQ.GROUND, keypoints=_np(d['keypoints']), scene2cam=TQ.SCENE2CAM, focal=TQ.CAM[:2],
                      center=TQ.CAM[2:], joints_ref=_np(d['joints_ref']), mask_ref=_np(d['mask_ref']), gap=_np(d['gap']))
    bare = track_quality(_np(d['joints']))
    clear = floor_clearance(G._d(seeded(3, 3, 7, 3)), 'z', -0.02, 0.05)
    return [('rows', q.rows), ('totals', torch.from_numpy(q.totals)), ('rows, joints only', bare.rows), ('clearance', clear)]


@xcase('floor[candidates N50, hypotheses P3 / P65, moments P3 / P65]')
def _floor():
    import test_gpu_floor as TF
    from rohm_amd.floor import floor_candidates, floor_hypotheses, floor_moments
    j, t, valid, kp = TF.make_track(50, 250)
    vi = np.flatnonzero(valid).astype(np.int32)
    out = [('flags', floor_candidates(_np(j), _np(t), _np(vi), _np(kp))), ('flags, no keypoints', floor_candidates(_np(j), _np(t), _np(vi)))]
    plane, origin = np.array([0.1, 0.0, -1.0, 3.0]) / np.sqrt(1.01), np.array([0.1, -0.2, 3.0])
    for case in ((3, 1, 1, 0), (65, 50, 64, 3)):
        pts, jts, tr = TF.make_hyp_inputs(*case)
        planes, scores, best = floor_hypotheses(_np(pts), _np(jts), _np(tr), TF.TAU, TF.UNDER)
        out += [(f'P{case[0]} planes', planes), (f'P{case[0]} scores', scores), (f'P{case[0]} best', best),
                (f'P{case[0]} moments', floor_moments(_np(pts), _np(plane), _np(origin), TF.TAU))]
    return out


@xcase('fit[pose N3 with normal equations, smoothed, shape moments]')
def _fit():
    import test_gpu_fit as TF
    from rohm_amd.body_model import SMPLXLayer, native_for
    from rohm_amd.fit import default_w_prior, fit_pose, shape_moments
    nat = native_for(SMPLXLayer.from_tensors(TF.tensors()).to(DEV), torch.device(DEV))
    joints, conf, b = TF.problem(3)
    wp = default_w_prior()
    p, r, n = fit_pose(nat, _np(joints), _np(conf), _np(b), w_prior=_np(wp), iters=3, want_normal=True)
    g = np.random.Generator(np.random.PCG64(303))
    start = np.concatenate([g.standard_normal((3, TF.NROT)) * 0.3, g.standard_normal((3, 3)) + (0, 0, 3.0)], axis=1)
    p2, r2, _ = fit_pose(nat, _np(joints), _np(conf), _np(b), init=_np(start), prev=_np(start), w_prior=_np(wp), w_smooth=0.01, iters=2)
    rows, out = shape_moments(nat, _np(joints), _np(conf), _np(start), _np(np.array([1, 1, 0], np.uint8)))
    return [('params', p), ('report', r), ('normal', n), ('params, smoothed', p2), ('report, smoothed', r2), ('moment rows', rows),
            ('moments', out)]


@xcase('export_smplx_blend[two candidates, one candidate, out-of-range frame]')
def _export_blend():
    from rohm_amd import ops
    from rohm_amd.body_model import native_for
    body = G._body().to(DEV)
    x, (mean, std) = G._repr_batch()                                       # [2, 294, 1, 20]
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    clip, row = i32([0, 0, 1, 1, 5, 0]), i32([0, 15, 3, 19, 0, 7])         # clip 5 does not exist: a NaN row
    clip_b, row_b = i32([-1, 1, 0, -1, 0, 1]), i32([0, 2, 16, 0, 1, 30])   # the last b candidate's row does not exist either
    alpha = torch.tensor([0.0, 0.25, 0.75, 0.0, 0.5, 0.5], dtype=torch.float64, device=DEV)
    transf = torch.eye(4, device=DEV).repeat(2, 1, 1).contiguous()
    transf[:, :3, 3] = torch.tensor([0.5, -1.0, 0.25], device=DEV)
    h = native_for(body, DEV).handle
    params, contact, dis = ops.export_smplx_blend(h, x, 'bc1t', clip, row, clip_b, row_b, alpha, transf=transf,
                                                  rigid=torch.eye(4, dtype=torch.float64, device=DEV), mean=_np(mean), std=_np(std))
    plain, none, none2 = ops.export_smplx_blend(h, x, 'bc1t', clip, row, clip_b, row_b, alpha, want_contact=False, want_disagree=False)
    assert none is None and none2 is None
    return [('params', params), ('contact', contact), ('disagree', dis), ('params, no transforms', plain)]


ALL = dict(G.CASES)
ALL.update(EXTRA)

# ================================================================================================ what the cases are allowed
# family -> {`*_bytes` function: why the wrapper asks for more than it returns}; these entry points are driven directly below
OVERSIZED = {
    'gemm_res_layernorm': {'rohm_gemm_res_layernorm_scratch_bytes': 'ops.gemm_res_layernorm adds 16 ints to align the scratch itself'},
    'output_process': {'rohm_output_process_scratch_bytes': 'ops.output_process adds 64 ints to align the scratch itself'},
}
# family -> the allocations a case may make past the guard, each with its reason (none today)
UNGUARDED = {}
# family -> labels of the outputs that ARE an input updated in place / labels of the canvases handed in to be updated
INPLACE = {'planes': {'layernorm'}, 'posenet_loop': {'x'}, 'trajnet_loop': {'x'}, 'train_helpers': {'trajectory window'}}
INPLACE_CANVAS = {'optim': {'#0', '#1', '#2', '#3'}}
PARAMS_ON_CANVASES = {'posenet_train': 22, 'trajnet_train': 186}       # family -> its fewest parameter tensors (L = 1; TrajNet without control)
NO_INPUT_THROUGH_D = {'track_resample': 'every input is a numpy array the wrapper uploads itself'}


_BASE, _ALIGNED = {}, {}


def _base(name):
    """(the case's outputs from plain zero-filled memory, whether a second such run repeats them bit for bit), computed once."""
    if name not in _BASE:
        fn = ALL[name]
        base = G._run(fn, SM.ZEROS)
        assert base and all(t.numel() > 0 for _, t in base)
        repeatable = not SM.differences(G._run(fn, SM.ZEROS), base)
        assert repeatable or name in G.ORACLE, f'{name}: two zero-filled runs differ and the case names no oracle'
        _BASE[name] = (base, repeatable)
    return _BASE[name]


def _hold_to_base(name, got, what):
    base, repeatable = _base(name)
    if repeatable:
        diff = SM.differences(got, base)
        assert not diff, f'{name}: {what} changes the result: {diff[:3]}'       # (output, (first differing element, value here, baseline))
    else:
        G.ORACLE[name](got)


@contextlib.contextmanager
def _byte_counts():
    """Record (function, value) of every `rohm_*_bytes` call made through `_lib.lib()` while active."""
    from rohm_amd import _lib
    handle, calls = _lib.lib(), []
    with pytest.MonkeyPatch.context() as m:
        for fname in _lib.SIGNATURES:
            if fname.endswith('_bytes'):
                def counted(*a, _real=getattr(handle, fname), _name=fname):
                    v = _real(*a)
                    calls.append((_name, int(v)))
                    return v
                m.setattr(handle, fname, counted)
        yield calls


def _byte_count_problems(name, g, calls):
    sizes = [r.nbytes for r in g.records]
    by_fn = {}
    for fname, v in calls:
        if v > 0:
            by_fn.setdefault(fname, set()).add(v)
    problems = []
    for fname, values in sorted(by_fn.items()):
        if fname in OVERSIZED.get(G.family(name), {}):
            continue
        exact = {v for v in values if v in sizes}
        for v in sorted(values - exact):
            if any(e >= v for e in exact):
                continue                                    # a handle that keeps its larger workspace of an earlier call
            near = sorted(s for s in sizes if v < s <= v + 65536)
            problems.append(f'{fname} returned {v}, no allocation has that size' + (f' (but there is one of {near[0]} bytes)' if near else ''))
    return problems


# ================================================================================================ (a), (b): outputs and workspaces
@pytest.mark.parametrize('name', sorted(ALL))
def test_no_access_outside_outputs_workspaces_scratch_and_saved_buffers(name):
    fn = ALL[name]
    _base(name)
    with GM.guard() as g, _byte_counts() as calls:
        got = SM.snapshot(fn())
        bad = g.violations()
    print(f'{name}: {g.served} guarded allocations, {sum(r.nbytes for r in g.records)} bytes, {g.unguarded} unguarded, '
          f'byte counts {sorted(set(calls))}')
    assert not bad, f'{name}: bytes outside an allocation were written: {bad[:5]} (index, allocation, offset of the first changed byte)'
    allowed = UNGUARDED.get(G.family(name), {})
    assert all(any(p.startswith(k) for k in allowed) for p in g.passed_through), f'{name}: allocations past the guard: {g.passed_through}'
    assert g.served > 0
    _hold_to_base(name, got, 'running between guard bands')
    problems = _byte_count_problems(name, g, calls)
    assert not problems, f'{name}: {problems}'


@pytest.mark.parametrize('M,N,K', ((288, 512, 64), (144, 1024, 32)))
def test_gemm_res_layernorm_in_a_scratch_of_exactly_the_stated_bytes(M, N, K):
    from rohm_amd import ops
    from rohm_amd._lib import lib
    args = G._ln_args(M, N, K)
    with SM.poison(SM.ZEROS):
        want = ops.gemm_res_layernorm(*args)
    nbytes = lib().rohm_gemm_res_layernorm_scratch_bytes(M, N)
    with GM.guard() as g:
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)       # 512-byte aligned: no trimming
        outs = [torch.empty(M, N, device=DEV) for _ in range(2)]
        for out in outs:                                                    # the second call meets the first one's armed header
            G._ln_call(args, scratch, nbytes, out)
        torch.cuda.synchronize()
        assert int(scratch[:4].view(torch.int32)) == 0, 'exchange error word'
        assert g.violations() == [] and g.served == 3 and g.records[0].nbytes == nbytes
    for out in outs:
        assert SM.first_difference(out, want) is None, SM.first_difference(out, want)


@pytest.mark.parametrize('B', (32, 3))
def test_output_process_in_a_scratch_of_exactly_the_stated_bytes(B):
    import math
    from rohm_amd import ops
    from rohm_amd._lib import check, lib, ptr, stream_ptr
    T, D, Cc = 143, 512, 272
    h, w, b = (G._d(t) for t in (seeded(B, B * (T + 1), D) * 2 + 0.1, seeded(B + 1, Cc, D) / math.sqrt(D), seeded(B + 2, Cc)))
    with SM.poison(SM.ZEROS):
        want = ops.output_process(h, w, b, B, T, ch_off=22, c_total=294)
    nbytes = lib().rohm_output_process_scratch_bytes()
    with GM.guard() as g:
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        out = torch.zeros(B, 294, 1, T, device=DEV)
        check(lib().rohm_output_process_f32(ptr(h), ptr(w), ptr(b), ptr(out), B, T, D, Cc, 22, 294, ptr(scratch), nbytes, stream_ptr(h.device)),
              'rohm_output_process_f32')
        torch.cuda.synchronize()
        assert int(scratch[:4].view(torch.int32)) == 0, 'stream-K exchange error word'
        assert g.violations() == [] and g.served == 2 and g.records[0].nbytes == nbytes
    assert SM.first_difference(out, want) is None, SM.first_difference(out, want)


# ================================================================================================ (c), (d): inputs
def _is_clip_batch(t):
    return t.dtype == torch.float32 and t.dim() in (4, 5) and tuple(t.shape[-3:-1]) == (294, 1)


def _placed_run(name, slices=False, offset=False):
    """Run the case with `_d` placing every input on a canvas ('slice' for the [.., 294, 1, T] float32 operands when `slices`, 'offset'
    for every operand when `offset`) and,
    for the training families, every parameter on a canvas of its own -> (outputs, canvases, the in-place canvases' labels)."""
    fn, fam = ALL[name], G.family(name)
    canv = []

    def d(t):
        label = f'#{len(canv)}'
        assert t.is_contiguous(), f'{name}: input {label} {tuple(t.shape)} is not contiguous and cannot be placed'
        if slices and _is_clip_batch(t):
            return GM.place(t.reshape(-1, 294, 1, t.shape[-1]), 'slice', device=DEV, into=canv, label=label).view(t.shape)
        return GM.place(t, 'offset' if offset else 'aligned', device=DEV, into=canv, label=label)

    def with_parameters_on_canvases(make):
        def made(*a, **k):
            net = make(*a, **k)
            for pname, q in net.named_parameters():
                if slices:      # a view into a flat buffer: one float past a 512-byte boundary
                    flat = torch.cat([q.data.reshape(-1)[:1], q.data.reshape(-1)])
                    q.data = GM.place(flat, 'aligned', into=canv, label='parameter ' + pname)[1:].view(q.shape)
                else:
                    q.data = GM.place(q.data, 'aligned', into=canv, label='parameter ' + pname)
            return net
        return made

    with pytest.MonkeyPatch.context() as m:
        m.setattr(G, '_d', d)
        if fam in PARAMS_ON_CANVASES:
            m.setattr(G, '_make_posenet', with_parameters_on_canvases(G._make_posenet))
            m.setattr(G, '_make_trajnet', with_parameters_on_canvases(G._make_trajnet))
        with SM.poison(SM.ZEROS):
            raw = fn()
            got = SM.snapshot(raw)
    at = {t.data_ptr() for label, t in raw if label in INPLACE.get(fam, ())}
    inplace = {c.label for c in canv if c.view.data_ptr() in at} | (INPLACE_CANVAS.get(fam, set()) & {c.label for c in canv})
    return got, canv, inplace


def _hold_canvases(name, canv, inplace):
    changed = {c.label for c in canv if not c.untouched()}
    detail = [(c.describe(), c.first_change()) for c in canv if c.label in changed - inplace]
    assert changed <= inplace, f'{name}: inputs were written: {detail[:5]} (canvas, offset of the first changed byte)'
    assert inplace <= changed, f'{name}: in-place operands {sorted(inplace - changed)} did not change'
    outside = [c.describe() for c in canv if not c.bands_untouched()]
    assert not outside, f'{name}: bytes around an input were written: {outside[:5]}'


def _aligned(name):
    if name not in _ALIGNED:
        _ALIGNED[name] = _placed_run(name)
    return _ALIGNED[name]


@pytest.mark.parametrize('name', sorted(ALL))
def test_no_access_outside_the_inputs(name):
    got, canv, inplace = _aligned(name)
    fam = G.family(name)
    print(f'{name}: {len(canv)} canvases, in place {sorted(inplace)}')
    assert all(c.view.data_ptr() % GM.ALIGN == 0 for c in canv)
    assert (len(canv) == 0) == (fam in NO_INPUT_THROUGH_D), (name, len(canv))
    if fam in PARAMS_ON_CANVASES:
        assert sum(c.label.startswith('parameter ') for c in canv) >= PARAMS_ON_CANVASES[fam]
    assert len(inplace) == len(INPLACE_CANVAS.get(fam, ())) + len(INPLACE.get(fam, ())), (name, sorted(inplace))
    _hold_to_base(name, got, 'placing the inputs between guard bands')
    _hold_canvases(name, canv, inplace)


SLICED = ([f'posenet_forward[chain {c}, B3, T143]' for c in ('0', 'layer', 'stack')] + ['posenet_forward[chain 0, B3, T63]'] +
          [f'posenet_loop[chain {c}, B3, T143, 8 steps]' for c in ('0', 'layer', 'stack')] +
          ['posenet_guided[amass, t 10]', 'ddpm[step, table, dropout mask]'] +
          [f'posenet_train[L1, B2, T63, dropout {p}]' for p in (0.0, 0.1)])
assert set(SLICED) <= set(ALL)


@pytest.mark.parametrize('name', SLICED)
def test_batch_slices_give_the_bits_of_the_aligned_run(name):
    want = _aligned(name)[0]
    got, canv, inplace = _placed_run(name, slices=True)
    sliced = [c for c in canv if c.placement == 'slice']
    print(f'{name}: {len(sliced)} of {len(canv)} inputs are batch slices')
    assert len(sliced) >= 2 and all(c.view.data_ptr() % 16 == 8 for c in sliced)
    if G.family(name) in PARAMS_ON_CANVASES:
        assert sum(c.label.startswith('parameter ') for c in canv) >= PARAMS_ON_CANVASES[G.family(name)]
    diff = SM.differences(got, want)
    assert not diff, f'{name}: a batch slice changes the result: {diff[:3]}'
    _hold_canvases(name, canv, inplace)


OFFSET = sorted(HC.CASES)      # the headers that promise in so many words that an operand "needs the alignment of its element only"


@pytest.mark.parametrize('name', OFFSET)
def test_operands_one_element_past_a_boundary_give_the_bits_of_the_aligned_run(name):
    """(d'): every input on an 'offset' canvas and every allocation of the wrappers from `guard(offset=True)` (which asserts the
    address of each): inputs, outputs and workspaces all start one element past a 512-byte boundary."""
    want = _aligned(name)[0]
    with GM.guard(offset=True) as g:
        got, canv, inplace = _placed_run(name, offset=True)
        bad = g.violations()
    print(f'{name}: {len(canv)} inputs and {g.served} allocations one element past a boundary')
    assert canv and all(c.placement == 'offset' and c.view.data_ptr() % GM.ALIGN == c.view.element_size() for c in canv)
    assert g.served > 0 and not g.passed_through, g.passed_through
    assert not bad, f'{name}: bytes outside an allocation were written: {bad[:5]}'
    diff = SM.differences(got, want)
    assert not diff, f'{name}: operands one element past a boundary change the result: {diff[:3]}'
    _hold_canvases(name, canv, inplace)


@pytest.mark.parametrize('name', sorted(HC.CASES))
def test_a_header_case_runs_every_declaration_of_its_header(name):
    """Counted through the loaded library: the case calls every function its header declares -- the host-only ones (rohm_mv_limits,
    the two `*_ws_bytes`) included, no exemptions -- and counting changes no result."""
    from rohm_amd import _lib
    declared = {f for f, _ in SM.declarations(SM.abi_headers()[HC.CASES[name][0]])}
    assert declared and declared <= set(_lib.SIGNATURES)
    handle, seen = _lib.lib(), set()
    with pytest.MonkeyPatch.context() as m:
        for fname in declared:
            def counted(*a, _real=getattr(handle, fname), _name=fname):
                seen.add(_name)
                return _real(*a)
            m.setattr(handle, fname, counted)
        got = G._run(ALL[name], SM.ZEROS)
    assert seen == declared, sorted(declared - seen)
    _hold_to_base(name, got, 'counting the calls')


# ================================================================================================ (e): the check can fail
def test_a_planted_overrun_is_reported():
    """rohm_ddpm_step told that its tensors are four floats longer than they are: it reads 16 bytes of the input canvases' bands (NaN)
    and stores four floats behind the output.  The only deliberate overrun of the module; every access stays inside the test's own
    allocations (1 MiB bands on either side of all four tensors), nothing faults.  The input bands carry the NaN 0x7FC00001, not
    all-ones: a NaN keeps its bits through the update, and all-ones stored onto the output's all-ones band would change nothing."""
    from rohm_amd._lib import check, lib, ptr, stream_ptr
    n, over = 3 * 294 * 143, 4
    canv = []
    x_t, x0, noise = (GM.place(seeded(s, n), 'aligned', device=DEV, into=canv, band=b'\x01\x00\xc0\x7f') for s in (1, 2, 3))
    with GM.guard() as g:
        out = torch.empty(n, device=DEV)
        check(lib().rohm_ddpm_step(ptr(x_t), ptr(x0), ptr(noise), None, 0.3, 0.7, 0.1, 0.0, ptr(out), n + over, stream_ptr(out.device)),
              'rohm_ddpm_step')
        bad = g.violations()
        behind = g.records[0].flat[g.records[0].front + 4 * n:][:4 * over].view(torch.float32).cpu()
    assert [(i, off) for i, _, off in bad] == [(0, 4 * n)], bad
    assert 'empty' in bad[0][1] and str(n) in bad[0][1]
    assert torch.isnan(behind).all(), behind
    want = 0.3 * x0 + 0.7 * x_t + 0.1 * noise
    assert torch.isfinite(out).all() and float((out - want).abs().max()) < 1e-5
    assert all(c.untouched() for c in canv)
