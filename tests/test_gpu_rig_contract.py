"""GPU: include/rohm_rig.h held to the four contracts of include/rohm_hip.h that its opening comment takes over -- a call touches
nothing outside its operands, results do not depend on what the outputs and workspaces held, every launch goes on the caller's
stream and nothing waits, and every stream-taking function records into a graph and replays.  The coverage tables of the existing
families (tests/stale_memory.py, stream_order.py, graph_replay.py, test_gpu_bounds.py) parse rohm_hip.h and do not see this header;
this file stands in for them, with their helpers, exactly as tests/test_gpu_multiview_contract.py does for rohm_multiview.h (whose
`Unaligned` it borrows: an operand one element past a 512-byte boundary between two bands of 0xFF bytes).

Every declaration of the header is run by `call` below, with no exemptions (`test_every_declaration_is_run`).  V = 4, N = 3, J = 22
(66 points: five tiles of the bundle adjustment, the last ragged), Q = 6 pairs, K = 5 hypotheses; salted inputs with one planted
outlier per point, a degenerate sample, a NaN point."""
import os

import numpy as np
import pytest
import torch

import graph_replay as GR
import multiview_ref as MR
import rig_ref as RR
import stale_memory as SM
import stream_order as SO
from test_gpu_multiview_contract import Unaligned, differences, snapshot

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
V, N, J, Q, K = 4, 3, 22, 6, 5
P = N * J
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'rohm_rig.h')
with open(HEADER) as _f:
    TEXT = _f.read()
POINTERS = SM.abi_pointer_functions(TEXT)
STREAMS = SO.abi_stream_functions(TEXT)
HOST_ONLY = {'rohm_rig_pair_ws_bytes', 'rohm_rig_ba_ws_bytes'}
MIN_REMAINING = 0.010                           # seconds of gate every call must find left
_INPUTS = {}


def inputs(seed):
    """{name: numpy array} of one value set: keypoints, the planted rig (disturbed), pairs, samples, the restatement's winning E, the
    planted points (disturbed, one NaN) and a camera step."""
    if seed not in _INPUTS:
        from rohm_amd.multiview import pack_cameras
        g = np.random.Generator(np.random.PCG64(seed + 9))
        Kc, W, D = MR.make_rig(V, seed, True, radius=3.0)
        cams = pack_cameras(Kc, W, D)
        kp, X = MR.make_views(cams, N, J, seed + 1, noise_px=2.0, spread=1.5)
        kp = MR.salt(MR.plant_outliers(kp, 1, seed + 2)[0], seed + 3)
        kp[1:, 1, :, 2] = 0.9                                              # salt() blinds frame 1; give it back to all but view 0
        cams[:, 9:12] += g.standard_normal((V, 3)) * 0.01
        pairs = np.stack(np.triu_indices(V, 1), 1).astype(np.int32)
        samples = RR.draw_samples(RR.undistorted(kp, cams), pairs, K, seed + 4, min_gap=4e-6)
        samples[0, 0, 3] = samples[0, 0, 1]                                # a repeated index
        ref = RR.pair_hypotheses(kp, cams, pairs, samples)
        E = np.stack([ref['E'][q, max(int(ref['best'][q]), 0)] for q in range(Q)])
        E[~np.isfinite(E).all(-1)] = 0.0
        points = X.reshape(P, 3) + g.standard_normal((P, 3)) * 0.01
        points[5] = np.nan
        _INPUTS[seed] = {'kp': kp, 'cams': cams, 'pairs': pairs, 'samples': samples, 'E': E, 'points': points, 'dc': g.standard_normal((V, 6)) * 1e-3}
    return _INPUTS[seed]


def call(t):
    """Every entry point of the header on the device tensors `t` -> [(label, tensor)]."""
    from rohm_amd import rig
    assert rig.pair_ws_bytes(V, P) == V * P * 16 and rig.ba_ws_bytes(V, P) > 0
    E, counts, best = rig.pair_hypotheses(t['kp'], t['cams'], t['pairs'], t['samples'])
    mom = rig.pair_moments(t['kp'], t['cams'], t['pairs'], t['E'])
    S, r, stats = rig.ba_moments(t['kp'], t['cams'], t['points'])
    Xn, cn = rig.ba_update(t['kp'], t['cams'], t['points'], t['dc'])
    return [('E_all', E), ('counts', counts), ('best', best), ('moments', mom), ('S', S), ('r', r), ('stats', stats), ('points_new', Xn),
            ('cams_new', cn)]


def on_device(seed, put=lambda t: t.to(DEV)):
    return {k: put(torch.from_numpy(np.array(a))) for k, a in inputs(seed).items()}


@pytest.fixture(scope='module')
def plain():
    with SM.poison(SM.ZEROS):
        return snapshot(call(on_device(7)))


# ---- coverage ------------------------------------------------------------------------------------------------------------------
def test_every_declaration_is_run(plain):
    from rohm_amd import _lib
    names = set(_lib.SIGNATURES_RIG)
    assert set(POINTERS) | HOST_ONLY == names and set(STREAMS) == names - HOST_ONLY == set(POINTERS)
    for name, at in STREAMS.items():                                        # the stream is the last parameter, as the ctypes table has it
        assert at == len(_lib.SIGNATURES_RIG[name][1]) - 1
    assert 'obey rohm_hip.h\'s "Conventions" and "Caller-owned memory" word for word' in SO.header_prose(TEXT)
    L, seen = _lib.lib(), []

    def counted(name, real):
        def f(*a):
            seen.append(name)
            return real(*a)
        return f
    real = {name: getattr(L, name) for name in names}
    try:
        for name in names:
            setattr(L, name, counted(name, real[name]))
        got = snapshot(call(on_device(7)))
    finally:
        for name in names:
            setattr(L, name, real[name])
    assert set(seen) == names
    assert not differences(got, plain)
    # the results are the restatement's: this file's inputs are held to it as tests/test_gpu_rig.py holds its own
    i = inputs(7)
    ref = RR.pair_hypotheses(i['kp'], i['cams'], i['pairs'], i['samples'])
    out = {k: v.cpu().numpy() for k, v in got}
    live = ref['counts'][..., 0] >= 0
    assert live.any() and (~live).any() and (ref['margin_tau'][live] >= 1e-6).all()
    assert np.array_equal(out['counts'], ref['counts']) and np.array_equal(out['best'], ref['best'])
    ok = RR.margins_ok(ref)
    assert ok.sum() >= 0.95 * live.sum() and np.abs(out['E_all'][ok] - ref['E'][ok]).max() <= 1e-9
    m = RR.ba_moments(i['kp'], i['cams'], i['points'])
    assert np.abs(out['S'] - m['S']).max() <= 1e-9 * np.abs(m['S']).max() and out['stats'][1] == m['n_obs']


# ---- nothing outside the operands -------------------------------------------------------------------------------------------------
def test_nothing_outside_the_operands_is_touched(plain):
    from rohm_amd import _lib, rig
    from rohm_amd._lib import check, ptr, stream_ptr
    L = _lib.lib()
    src = on_device(7)
    ops = {k: Unaligned(tuple(t.shape), t.dtype, t, k) for k, t in src.items()}
    f64, words = torch.float64, lambda nbytes: ((nbytes + 7) // 8,)
    for k, shape, dtype in (('E_all', (Q, K, 9), f64), ('counts', (Q, K, 2), torch.int64), ('best', (Q,), torch.int32), ('moments', (Q, 47), f64),
                            ('S', (6 * V, 6 * V), f64), ('r', (6 * V,), f64), ('stats', (2,), f64), ('points_new', (P, 3), f64),
                            ('cams_new', (V, 24), f64), ('ws_hyp', words(rig.pair_ws_bytes(V, P)), f64),
                            ('ws_mom', words(rig.pair_ws_bytes(V, P)), f64), ('ws_ba', words(rig.ba_ws_bytes(V, P)), f64)):
        ops[k] = Unaligned(shape, dtype, None, k)
    o = {k: c.view for k, c in ops.items()}
    s = stream_ptr(torch.device(DEV))
    check(L.rohm_rig_pair_hypotheses(ptr(o['kp']), ptr(o['cams']), ptr(o['pairs']), ptr(o['samples']), V, N, J, Q, K, 0.2, 4.0, ptr(o['ws_hyp']),
                                     ptr(o['E_all']), ptr(o['counts']), ptr(o['best']), s), 'rohm_rig_pair_hypotheses')
    check(L.rohm_rig_pair_moments(ptr(o['kp']), ptr(o['cams']), ptr(o['pairs']), ptr(o['E']), V, N, J, Q, 0.2, 4.0, ptr(o['ws_mom']), ptr(o['moments']),
                                  s), 'rohm_rig_pair_moments')
    check(L.rohm_rig_ba_moments(ptr(o['kp']), ptr(o['cams']), ptr(o['points']), V, N, J, 0.2, 10.0, 1e-3, ptr(o['ws_ba']), ptr(o['S']), ptr(o['r']),
                                ptr(o['stats']), s), 'rohm_rig_ba_moments')
    check(L.rohm_rig_ba_update(ptr(o['kp']), ptr(o['cams']), ptr(o['points']), ptr(o['dc']), V, N, J, 0.2, 10.0, 1e-3, ptr(o['points_new']),
                               ptr(o['cams_new']), s), 'rohm_rig_ba_update')
    torch.cuda.synchronize()
    for k, c in ops.items():
        assert c.bands_untouched(), f'{k}: a byte outside the operand was written'
        if c.is_input:
            assert c.untouched(), f'{k}: an input was written'
    got = [(label, o[label]) for label, _ in plain]
    assert not differences(got, plain)                                      # ... and unaligned operands give the aligned ones' bits
    # cams_new NULL is not computed, and nothing else changes
    before = ops['points_new'].flat.clone()
    check(L.rohm_rig_ba_update(ptr(o['kp']), ptr(o['cams']), ptr(o['points']), ptr(o['dc']), V, N, J, 0.2, 10.0, 1e-3, ptr(o['points_new']), None, s),
          'rohm_rig_ba_update')
    torch.cuda.synchronize()
    assert torch.equal(ops['points_new'].flat, before)


# ---- outputs and workspaces may hold anything ----------------------------------------------------------------------------------------
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
    assert log.functions() == set(STREAMS) and len(log.calls) == 4
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
