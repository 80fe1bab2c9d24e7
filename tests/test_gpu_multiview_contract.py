"""GPU: include/rohm_multiview.h held to the four contracts of include/rohm_hip.h that its opening comment takes over -- a call
touches nothing outside its operands, results do not depend on what the outputs held, every launch goes on the caller's stream
and nothing waits, and every stream-taking function records into a graph and replays.  The coverage tables of the existing
families (tests/stale_memory.py, stream_order.py, graph_replay.py, test_gpu_bounds.py) parse rohm_hip.h and do not see this
header; this file stands in for them, with their helpers: the parsers (`text=`), `stream_order.CallLog` / `Gates` /
`DeferredInputs`, `graph_replay.Slots` / `run_case` (`lib_obj`, `stream_at`), `stale_memory.poison` / `PATTERNS`.

Every declaration of the header that takes a stream or a pointer to numbers is run by `call` below, with no exemptions
(`test_every_declaration_is_run`).  V = 4, N = 3, J = 22, salted inputs with one planted outlier per point.

One helper could not serve unedited: `guarded_memory.Canvas` places an operand on a 512-byte boundary (or as the batch slice of
a [B, 294, 1, T] tensor).  `Unaligned` below is its minimal equivalent with the operand one element past a 512-byte boundary --
4 bytes (float32, uint32) or 8 bytes (float64) past a 16-byte boundary -- between two bands of guarded_memory.BAND 0xFF bytes."""
import os

import numpy as np
import pytest
import torch

import graph_replay as GR
import guarded_memory as GM
import multiview_ref as MR
import stale_memory as SM
import stream_order as SO

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
V, N, J = 4, 3, 22
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'rohm_multiview.h')
with open(HEADER) as _f:
    TEXT = _f.read()
POINTERS = SM.abi_pointer_functions(TEXT)
STREAMS = SO.abi_stream_functions(TEXT)
MIN_REMAINING = 0.010                           # seconds of gate every call must find left (the calls here take some 0.02 ms of host time)
_INPUTS = {}


def inputs(seed):
    """{name: numpy array} of one value set: keypoints, cams, rigid, and world joints for the residuals (the restatement's, so that
    `rohm_mv_residuals` has an input of its own)."""
    if seed not in _INPUTS:
        from rohm_amd.multiview import pack_cameras
        K, W, D = MR.make_rig(V, seed, True)
        cams = pack_cameras(K, W, D)
        kp, _ = MR.make_views(cams, N, J, seed + 1, noise_px=2.0)
        kp = MR.salt(MR.plant_outliers(kp, 1, seed + 2)[0], seed + 3)
        rigid = np.concatenate([W[1, :3, :3].reshape(9), W[1, :3, 3]])
        world = MR.triangulate(kp, cams)['joints']
        _INPUTS[seed] = {'kp': kp, 'cams': cams, 'rigid': rigid, 'world': world}
    return _INPUTS[seed]


def call(t):
    """Every entry point of the header on the device tensors `t` -> [(label, tensor)]."""
    from rohm_amd import multiview
    assert multiview.limits() == (16, 120)
    a = multiview.triangulate(t['kp'], t['cams'], rigid=t['rigid'], want_undistorted=True)
    b = multiview.triangulate(t['kp'], t['cams'], min_views=3, refine=1)               # rigid and keypoints_und NULL
    r = multiview.view_residuals(t['world'], t['kp'], t['cams'])
    return [('joints', a.joints), ('conf', a.conf), ('report', a.report), ('inliers', a.inliers), ('keypoints_und', a.keypoints_und),
            ('joints_world', b.joints), ('conf_3', b.conf), ('report_3', b.report), ('inliers_3', b.inliers), ('resid', r)]


def on_device(seed, put=lambda t: t.to(DEV)):
    return {k: put(torch.from_numpy(np.array(a))) for k, a in inputs(seed).items()}


def snapshot(out):
    torch.cuda.synchronize()
    return [(label, t.detach().clone()) for label, t in out]


def differences(got, want):
    assert [l for l, _ in got] == [l for l, _ in want]
    return [(label, d) for (label, a), (_, b) in zip(got, want) for d in [SM.first_difference(a, b)] if d is not None]


@pytest.fixture(scope='module')
def plain():
    with SM.poison(SM.ZEROS):
        return snapshot(call(on_device(7)))


# ---- coverage ------------------------------------------------------------------------------------------------------------------
def test_every_declaration_is_run(plain):
    from rohm_amd import _lib
    assert set(POINTERS) == {'rohm_mv_limits', 'rohm_mv_triangulate', 'rohm_mv_residuals'} == set(_lib.SIGNATURES_MULTIVIEW)
    assert set(STREAMS) == {'rohm_mv_triangulate', 'rohm_mv_residuals'}
    for name, at in STREAMS.items():                                        # the stream is the last parameter, as the ctypes table has it
        assert at == len(_lib.SIGNATURES_MULTIVIEW[name][1]) - 1
    assert 'obey rohm_hip.h\'s "Conventions" and "Caller-owned memory" word for word' in SO.header_prose(TEXT)
    L, seen = _lib.lib(), []

    def counted(name, real):
        def f(*a):
            seen.append(name)
            return real(*a)
        return f
    real = {name: getattr(L, name) for name in POINTERS}
    try:
        for name in POINTERS:
            setattr(L, name, counted(name, real[name]))
        got = snapshot(call(on_device(7)))
    finally:
        for name in POINTERS:
            setattr(L, name, real[name])
    assert set(seen) == set(POINTERS) | set(STREAMS)
    assert not differences(got, plain)
    # the results are the restatement's: this file's inputs are held to it as tests/test_gpu_multiview.py holds its own
    ref = MR.triangulate(inputs(7)['kp'], inputs(7)['cams'], rigid=inputs(7)['rigid'])
    assert len(MR.margins_ok(ref)) == 0
    out = dict(got)
    assert np.array_equal(out['inliers'].cpu().numpy().astype(np.int64), ref['inliers'].astype(np.int64))
    has = ref['report'][..., 0] > 0
    d = np.abs(out['joints'].cpu().numpy()[has] - ref['joints'][has]).max(-1) / np.maximum(1.0, np.linalg.norm(ref['joints'][has], axis=-1))
    assert has.any() and (~has).any() and d.max() <= 1e-9


# ---- nothing outside the operands -------------------------------------------------------------------------------------------------
class Unaligned:
    """A flat buffer of 0xFF bytes holding one operand one element past a 512-byte boundary, GM.BAND bytes on either side."""

    def __init__(self, shape, dtype, value=None, label=''):
        item = torch.empty((), dtype=dtype).element_size()
        self.nbytes = int(np.prod(shape)) * item
        self.flat = torch.full((GM.BAND + GM.ALIGN + item + self.nbytes + GM.BAND,), 0xFF, dtype=torch.uint8, device=DEV)
        self.front = GM.BAND + (-(self.flat.data_ptr() + GM.BAND)) % GM.ALIGN + item
        self.view = self.flat[self.front:self.front + self.nbytes].view(dtype).view(shape)
        assert self.view.data_ptr() % 16 == item and self.view.is_contiguous()
        if value is not None:
            self.view.copy_(value)
        self.label, self.is_input = label, value is not None
        self.copy = self.flat.clone()

    def bands_untouched(self):
        a, b = self.front, self.front + self.nbytes
        return bool((self.flat[:a] == 0xFF).all()) and bool((self.flat[b:] == 0xFF).all())

    def untouched(self):
        return bool(torch.equal(self.flat, self.copy))


def test_nothing_outside_the_operands_is_touched(plain):
    from rohm_amd import _lib
    from rohm_amd._lib import check, ptr, stream_ptr
    L = _lib.lib()
    src = on_device(7)
    ops = {k: Unaligned(tuple(t.shape), t.dtype, t, k) for k, t in src.items()}
    for k, shape, dtype in (('joints', (N, J, 3), torch.float64), ('conf', (N, J), torch.float32), ('report', (N, J, 4), torch.float64),
                            ('inliers', (N, J), torch.int32), ('keypoints_und', (V, N, J, 3), torch.float32), ('joints_world', (N, J, 3), torch.float64),
                            ('conf_3', (N, J), torch.float32), ('report_3', (N, J, 4), torch.float64), ('inliers_3', (N, J), torch.int32),
                            ('resid', (V, N, J), torch.float64)):
        ops[k] = Unaligned(shape, dtype, None, k)
    o = {k: c.view for k, c in ops.items()}
    s, ang = stream_ptr(torch.device(DEV)), float(np.deg2rad(2.0))
    check(L.rohm_mv_triangulate(ptr(o['kp']), ptr(o['cams']), ptr(o['rigid']), V, N, J, 0.2, 10.0, ang, 2, 3, ptr(o['joints']), ptr(o['conf']),
                                ptr(o['report']), ptr(o['inliers']), ptr(o['keypoints_und']), s), 'rohm_mv_triangulate')
    check(L.rohm_mv_triangulate(ptr(o['kp']), ptr(o['cams']), None, V, N, J, 0.2, 10.0, ang, 3, 1, ptr(o['joints_world']), ptr(o['conf_3']),
                                ptr(o['report_3']), ptr(o['inliers_3']), None, s), 'rohm_mv_triangulate')
    check(L.rohm_mv_residuals(ptr(o['world']), ptr(o['kp']), ptr(o['cams']), V, N, J, 0.2, ptr(o['resid']), s), 'rohm_mv_residuals')
    torch.cuda.synchronize()
    for k, c in ops.items():
        assert c.bands_untouched(), f'{k}: a byte outside the operand was written'
        if c.is_input:
            assert c.untouched(), f'{k}: an input was written'
    got = [(label, o[label]) for label, _ in plain]
    assert not differences(got, plain)                                      # ... and unaligned operands give the aligned ones' bits


# ---- outputs may hold anything ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pattern', list(SM.PATTERNS))
def test_results_do_not_depend_on_what_the_outputs_held(pattern, plain):
    with SM.poison(SM.PATTERNS[pattern]):
        got = snapshot(call(on_device(7)))
    assert not differences(got, plain)


# ---- the caller's stream, and no wait -------------------------------------------------------------------------------------------------
def test_calls_return_behind_a_closed_gate(plain):
    from rohm_amd import _lib
    L = _lib.lib()
    side = torch.cuda.Stream()
    delay, guess = SO.torch_delay()
    rate = 1.25 * SO.calibrate(delay, guess, side)
    deferred = SO.DeferredInputs(DEV)
    on_device(7, deferred.record)                                           # the plain run's inputs, noted
    with torch.cuda.stream(side):
        deferred.stage()
    torch.cuda.synchronize()                                                # the pre-fills are written before any gate is armed
    gates = SO.Gates(side, 2.0 * MIN_REMAINING, delay, rate)
    log = SO.CallLog(gates, MIN_REMAINING)
    arm = lambda: gates.ensure_gate(MIN_REMAINING)
    try:
        with torch.cuda.stream(side), log.installed(L, STREAMS), SM.poison(SO.ONES):
            gates.arm()
            out = call(on_device(7, lambda t: deferred.replay(t, arm)))     # the values arrive behind the gate, on the side stream
    finally:
        torch.cuda.synchronize()
    assert deferred.complete()
    assert log.functions() == set(STREAMS) and len(log.calls) == 3
    assert not log.unproven(), f'calls returned with the gate open: {[(f, f"{1e3 * s:.3f} ms") for f, s in log.unproven()]}'
    assert log.proven() == set(STREAMS)
    assert not differences(snapshot(out), plain)


# ---- recordable -------------------------------------------------------------------------------------------------------------------------
def test_recorded_calls_replay_on_rewritten_inputs():
    from rohm_amd import _lib
    side = torch.cuda.Stream()
    slots = GR.Slots(DEV)
    for k in inputs(7):
        slots.add(k, torch.from_numpy(np.array(inputs(7)[k])), torch.from_numpy(np.array(inputs(8)[k])))
    r = GR.run_case(slots, lambda s, h: call({k: s[k] for k in inputs(7)}), host=lambda: None, rewrite=lambda h: None, side=side,
                    claims=set(STREAMS), lib_obj=_lib.lib(), stream_at=STREAMS)
    assert r['replays'] >= 3 and r['log'].recorded() == set(STREAMS)
    with SM.poison(SM.ZEROS):
        fresh = snapshot(call(on_device(7)))
    assert not differences([(label, t) for label, t in r['final']], fresh)  # the last replay, on set 1, against a fresh call
