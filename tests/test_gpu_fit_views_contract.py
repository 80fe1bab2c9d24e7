"""GPU: include/rohm_fit_views.h held to the four contracts of include/rohm_hip.h that its opening comment takes over -- a call
touches nothing outside its operands, results do not depend on what the outputs held, every launch goes on the caller's stream
and nothing waits, and every stream-taking function records into a graph and replays.  The coverage tables of the existing
families (tests/stale_memory.py, stream_order.py, graph_replay.py, test_gpu_bounds.py) parse rohm_hip.h and do not see this
header; this file stands in for them, with their helpers, as tests/test_gpu_multiview_contract.py does for its header (whose
`Unaligned` -- an operand one element past a 512-byte boundary between two guard bands -- is used here as it is).

Every declaration of the header is run by `call` below, with no exemptions (`test_every_declaration_is_run`): once with every
optional operand (prev, resid, normal; robust, smoothed) and once with all three NULL (plain).  V = 3, N = 3, peppered inputs
with an unusable middle frame, view 0 distorted, the start translation solved by the kernel."""
import os

import numpy as np
import pytest
import torch

import fit_ref as FR
import fit_views_ref as VR
import graph_replay as GR
import stale_memory as SM
import stream_order as SO
from rohm_amd.utils import synth
from test_gpu_multiview_contract import Unaligned

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
V, N, NJ, NX = 3, 3, VR.NJ, VR.NX
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'rohm_fit_views.h')
with open(HEADER) as _f:
    TEXT = _f.read()
POINTERS = SM.abi_pointer_functions(TEXT)
STREAMS = SO.abi_stream_functions(TEXT)
MIN_REMAINING = 0.010                           # seconds of gate every call must find left
SCALARS = ((700.0, 900.0, 30.0, 0.2, 3, 12), (0.0, 0.0, 0.0, 0.2, 2, 12))       # w_smooth, w_smooth_t, sigma_px, conf_min, iters, min_obs
_INPUTS, _CACHE = {}, {}


def tensors():
    if 'tensors' not in _CACHE:
        _CACHE['tensors'] = synth.synthetic_smplx_tensors(0)
    return _CACHE['tensors']


def nat():
    from rohm_amd.body_model import SMPLXLayer, native_for
    if 'layer' not in _CACHE:
        _CACHE['layer'] = SMPLXLayer.from_tensors(tensors()).to(DEV)
    return native_for(_CACHE['layer'], torch.device(DEV))


def inputs(seed):
    """{name: numpy array} of one value set."""
    if seed not in _INPUTS:
        from rohm_amd.fit_views import default_w_prior
        cams = VR.make_rig(V, seed, distorted=(0,))
        joints, truth, betas = VR.make_body(tensors(), N, seed + 1, root_base=VR.facing(cams), root_angle=0.6, beta_scale=0.5)
        kp = VR.pepper(VR.make_keypoints(cams, joints, seed + 2, conf=(0.3, 1.0)), seed + 3, dead_frame=1)
        g = np.random.Generator(np.random.PCG64(seed + 4))
        init = truth.copy()
        init[:, :VR.NROT] += g.standard_normal((N, VR.NROT)) * 0.05
        init[:, VR.NROT:] = np.nan
        _INPUTS[seed] = {'kp': kp, 'cams': cams, 'betas': np.repeat(betas[None].astype(np.float32), N, axis=0), 'init': init,
                         'prev': truth + 0.01, 'w_prior': default_w_prior(V)}
    return _INPUTS[seed]


def call(t):
    """Every entry point of the header on the device tensors `t` -> [(label, tensor)]."""
    from rohm_amd.fit_views import fit_views_pose
    ws, wst, sigma, conf_min, iters, min_obs = SCALARS[0]
    a = fit_views_pose(nat(), t['kp'], t['cams'], t['betas'], t['init'], prev=t['prev'], w_prior=t['w_prior'], w_smooth=ws, w_smooth_t=wst,
                       sigma_px=sigma, conf_min=conf_min, iters=iters, min_obs=min_obs, want_normal=True)
    ws, wst, sigma, conf_min, iters, min_obs = SCALARS[1]
    b = fit_views_pose(nat(), t['kp'], t['cams'], t['betas'], t['init'], w_prior=t['w_prior'], sigma_px=sigma, conf_min=conf_min, iters=iters,
                       min_obs=min_obs, want_resid=False)                  # prev, resid and normal NULL
    return [('params', a[0]), ('report', a[1]), ('resid', a[2]), ('normal', a[3]), ('params_plain', b[0]), ('report_plain', b[1])]


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
    nat()                                                                   # the body model handle is set up (and synchronises) here, once
    with SM.poison(SM.ZEROS):
        return snapshot(call(on_device(7)))


# ---- coverage ------------------------------------------------------------------------------------------------------------------
def test_every_declaration_is_run(plain):
    from rohm_amd import _lib
    assert set(POINTERS) == {'rohm_fit_views_pose'} == set(_lib.SIGNATURES_FIT_VIEWS) == set(STREAMS)
    for name, at in STREAMS.items():                                        # the stream is the last parameter, as the ctypes table has it
        assert at == len(_lib.SIGNATURES_FIT_VIEWS[name][1]) - 1
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
    assert set(seen) == set(POINTERS) and len(seen) == 2
    assert not differences(got, plain)
    # the results are the restatement's: this file's inputs are held to it as tests/test_gpu_fit_views.py holds its own
    i, out = inputs(7), dict(got)
    mdl = FR.model(tensors())
    ws, wst, sigma, conf_min, iters, min_obs = SCALARS[0]
    pw, rw, sw, nw = VR.fit_views_pose(mdl, i['kp'], i['cams'], i['betas'], i['init'], prev=i['prev'], w_prior=i['w_prior'], w_smooth=ws, w_smooth_t=wst,
                                       sigma_px=sigma, conf_min=conf_min, iters=iters, min_obs=min_obs, want_normal=True)
    r, n = out['report'].cpu().numpy(), out['normal'].cpu().numpy()
    assert rw[:, 0].tolist() == [1, 0, 1] and np.array_equal(r[:, 0], rw[:, 0]) and np.array_equal(r[:, 6], rw[:, 6])
    for f in (0, 2):
        assert np.abs(n[f] - nw[f]).max() <= 1e-9 * np.abs(nw[f]).max() and abs(r[f, 1] - rw[f, 1]) <= 1e-9 * rw[f, 1]
        assert r[f, 2] <= r[f, 1] and r[f, 2] <= 1.05 * rw[f, 2]


# ---- nothing outside the operands -------------------------------------------------------------------------------------------------
def test_nothing_outside_the_operands_is_touched(plain):
    from rohm_amd import _lib
    from rohm_amd._lib import check, ptr, stream_ptr
    L = _lib.lib()
    src = on_device(7)
    ops = {k: Unaligned(tuple(t.shape), t.dtype, t, k) for k, t in src.items()}
    for k, shape in (('params', (N, NX)), ('report', (N, 8)), ('resid', (V, N, NJ)), ('normal', (N, NX, NX + 1)), ('params_plain', (N, NX)),
                     ('report_plain', (N, 8))):
        ops[k] = Unaligned(shape, torch.float64, None, k)
    o = {k: c.view for k, c in ops.items()}
    s, h = stream_ptr(torch.device(DEV)), nat().handle
    ws, wst, sigma, conf_min, iters, min_obs = SCALARS[0]
    check(L.rohm_fit_views_pose(h, ptr(o['kp']), ptr(o['cams']), ptr(o['betas']), ptr(o['init']), ptr(o['prev']), ptr(o['w_prior']), ws, wst, sigma,
                                conf_min, iters, min_obs, V, N, ptr(o['params']), ptr(o['report']), ptr(o['resid']), ptr(o['normal']), s),
          'rohm_fit_views_pose')
    ws, wst, sigma, conf_min, iters, min_obs = SCALARS[1]
    check(L.rohm_fit_views_pose(h, ptr(o['kp']), ptr(o['cams']), ptr(o['betas']), ptr(o['init']), None, ptr(o['w_prior']), ws, wst, sigma, conf_min,
                                iters, min_obs, V, N, ptr(o['params_plain']), ptr(o['report_plain']), None, None, s), 'rohm_fit_views_pose')
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
    assert log.functions() == set(STREAMS) and len(log.calls) == 2
    assert not log.unproven(), f'calls returned with the gate open: {[(f, f"{1e3 * s:.3f} ms") for f, s in log.unproven()]}'
    assert log.proven() == set(STREAMS)
    assert not differences(snapshot(out), plain)


# ---- recordable -------------------------------------------------------------------------------------------------------------------------
def test_recorded_calls_replay_on_rewritten_inputs(plain):
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
