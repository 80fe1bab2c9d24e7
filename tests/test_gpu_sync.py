"""GPU: camera synchronisation -- `rohm_sync_pair_sweep` and `rohm_sync_resample` (csrc/sync.hip, include/provisional/rohm_sync.h)
against their float64 restatement (tests/sync_ref.py, held to tests/rig_ref.py, closed forms and planted offsets in
tests/test_sync_ref.py), the contracts the provisional header claims -- the contract families of tests/ read the registries of
`_lib.HEADERS` only, so this module holds the two entry points to them itself -- and `python -m rohm_amd.sync` -> `python -m
rohm_amd.rig` end to end.

Shapes (`sync_ref.SWEEP_CASES`).  (V, N, J, Q, S) = (2, 3, 22, 1, 7): shifts beyond +-N and empty overlaps, once with a finite E and
once with the one pair's E not finite; (4, 70, 25, 6, 33): P = 1 750, seven strides per thread, the last ragged; (16, 5, 22, 120, 3):
every pair of 16 views.  Each has integer, negative and fractional shifts and one NaN shift per pair, salted keypoints (NaN and
infinite coordinates; zero, negative and NaN confidences), a pair outside [0, V) and one with v1 = v2 where Q allows, and an E that
is not finite in one pair.

Bars.  Kernel and restatement are both float64 on the same float32 inputs.  The counts and the NaN / zero pattern are EQUAL; that
rests on no |d - tau_px| < 1e-6 px and no interpolation index within 1e-9 of an integer (other than exactly on one), which
tests/test_sync_ref.py::test_margins_of_the_gpu_inputs asserts on the CPU for every case and `_margins` asserts here once per
session.  The two sums: 1e-9 of the operand's largest magnitude, `rig`'s bar.  The resampler: 0 float32 ulp -- its two products and
one sum are each rounded, in the kernel as in numpy.  The largest measured values go to profiles/sync_parity.json (group `gpu`).

End to end.  V = 3, N = 40, J = 22, planted offsets (0, +1.37, -2.6) frames, 0.5 px of noise, --max_offset_s covering 5 frames, 64
hypotheses, 6 rounds (three alternations have not converged at N = 40: 0.04 frame on the restatement, six give 0.01).  The offset
bars are twice the restatement's own error on this scene (`sync_ref.END_TO_END_BARS`, measured in tests/test_sync_ref.py).  The seed
was chosen with the restatement on the CPU: of the seeds 811 to 814 all four put `rig` on the synchronised output within
tests/test_gpu_rig.py's bars (rotation 0.04, 0.02, 0.10, 0.08 degrees; centre 4.8, 1.0, 5.6, 6.4 mm); 811 is the first."""
import contextlib
import ctypes as C
import json

import numpy as np
import pytest
import torch

import rig_ref as RR
import stale_memory as SM
import sync_ref as SR

record = SR.record
pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BAR = 1e-9
CANARY = b'\xa5\x5a\xc3\x3c'


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                           # a copy: the shared inputs are read-only


@pytest.fixture(scope='session')
def _margins():
    for name in SR.SWEEP_CASES:
        case = SR.build_sweep_case(name)
        assert (case['margin_tau'] >= 1e-6).all() and (case['margin_index'] >= 1e-9).all(), name


def sweep(case):
    from rohm_amd import sync
    return sync.pair_sweep(*(_dev(case[k]) for k in ('keypoints', 'cams', 'pairs', 'E', 'shifts')))


@pytest.mark.parametrize('name', list(SR.SWEEP_CASES))
def test_pair_sweep_matches_the_restatement(name, _margins):
    case = SR.build_sweep_case(name)
    want = case['ref']
    got = sweep(case).cpu().numpy()
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))                   # the NaN pattern
    live = np.isfinite(want).all(-1)
    assert live.any() and (~live).any()
    assert np.array_equal(got[live][:, :2], want[live][:, :2])             # the counts, and with them the zero pattern
    assert np.array_equal(got[live] == 0, want[live] == 0)
    d = max((np.abs(got[live][:, k] - want[live][:, k]) / np.maximum(np.abs(want[live][:, k]), 1.0)).max() for k in (2, 3))
    print(f'{name}: sums {d:.3e} relative over {int(live.sum())} live (pair, shift) cells; common up to {int(want[live][:, 0].max())}, '
          f'inliers up to {int(want[live][:, 1].max())}, {int((want[live][:, 0] == 0).sum())} empty')
    record('gpu', 'sweep_sums_rel', d)
    assert d <= BAR


@pytest.mark.parametrize('sigma_px', [0.0, 10.0])
def test_pair_sweep_at_other_parameters(sigma_px, _margins):
    """sigma_px = 0 (the plain sum, +inf under an E that is not finite) and another tau_px, on the many-points case."""
    from rohm_amd import sync
    case = SR.build_sweep_case('many_points')
    args = [case[k] for k in ('keypoints', 'cams', 'pairs', 'E', 'shifts')]
    want, mt, _ = SR.pair_sweep(*args, tau_px=7.0, sigma_px=sigma_px, with_margins=True)
    assert (mt >= 1e-6).all()
    got = sync.pair_sweep(*(_dev(a) for a in args), tau_px=7.0, sigma_px=sigma_px).cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
    assert np.isinf(want).any() == (sigma_px == 0.0)
    ok = np.isfinite(want)
    assert np.array_equal(got[..., :2][ok[..., :2]], want[..., :2][ok[..., :2]])
    assert (np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), 1.0)).max() <= BAR


@pytest.mark.parametrize('name', list(SR.SWEEP_CASES))
def test_resampler_matches_the_restatement_bit_for_bit(name):
    from rohm_amd import sync
    case = SR.build_resample_case(name)
    got = sync.resample_views(_dev(case['keypoints']), _dev(case['shifts'])).cpu().numpy()
    want = case['ref']
    assert got.dtype == np.float32 and got.shape == want.shape
    differ = got.view(np.uint32) != want.view(np.uint32)
    print(f'{name}: {int(differ.sum())} of {differ.size} float32 values differ; shifts {np.round(case["shifts"], 3).tolist()}')
    record('gpu', 'resample_values_that_differ', differ.sum())
    assert not differ.any()
    assert np.array_equal(got[0].view(np.uint32), case['keypoints'][0].view(np.uint32))            # shift 0: the view's bits


def everything(pattern=None):
    """Both kernels on the many-points and the sixteen-views cases -> [(label, tensor)]; under `pattern` the outputs and the workspace
    are poisoned first."""
    from rohm_amd import sync
    out = []
    with (SM.poison(pattern) if pattern is not None else contextlib.nullcontext()):
        for name in ('many_points', 'sixteen_views'):
            out.append((name + ' sweep', sweep(SR.build_sweep_case(name))))
            rs = SR.build_resample_case(name)
            out.append((name + ' resample', sync.resample_views(_dev(rs['keypoints']), _dev(rs['shifts']))))
        torch.cuda.synchronize()
    return out


def test_the_same_bits_twice_and_over_poisoned_memory():
    first = everything()
    for pattern in [None] + list(SM.PATTERNS.values()):
        assert not SM.differences(everything(pattern), first), pattern


# ---- bounds ---------------------------------------------------------------------------------------------------------------------------
def _placed(t, canvases):
    """A copy of the CPU tensor `t` on the device as a slice of a larger canary-filled tensor, its first element one element past a
    512-byte boundary."""
    es = t.element_size()
    lead, n = 512 // es + 1, t.numel()
    big = torch.empty(lead + n + 512 // es, dtype=t.dtype, device=DEV)
    SM.fill_bytes(big, CANARY)
    assert big.data_ptr() % 512 == 0
    big[lead:lead + n] = t.reshape(-1).to(DEV)
    canvases.append((big, lead, n, SM.bits(big).clone()))
    return big[lead:lead + n].view(t.shape)


def _canaries_intact(canvases, outputs=()):
    """Every guard band keeps its canaries; every operand that is not an output keeps its bits too."""
    for k, (big, lead, n, before) in enumerate(canvases):
        es = big.element_size()
        after = SM.bits(big)
        assert torch.equal(after[:lead * es], before[:lead * es]) and torch.equal(after[(lead + n) * es:], before[(lead + n) * es:]), k
        if k not in outputs:
            assert torch.equal(after, before), k


@pytest.mark.parametrize('name', ['one_pair', 'many_points'])
def test_operands_one_element_past_an_aligned_boundary_between_canaries(name):
    from rohm_amd import _lib, sync
    from rohm_amd._lib import check, ptr, stream_ptr
    case, rs = SR.build_sweep_case(name), SR.build_resample_case(name)
    V, N, J = case['keypoints'].shape[:3]
    Q, S = case['shifts'].shape
    want = sweep(case)
    want_rs = sync.resample_views(_dev(rs['keypoints']), _dev(rs['shifts']))
    canv = []
    kp, cams, pairs, E, sh = (_placed(torch.from_numpy(np.array(case[k])), canv) for k in ('keypoints', 'cams', 'pairs', 'E', 'shifts'))
    ws = _placed(torch.zeros(sync.ws_bytes(V, N * J) // 8, dtype=torch.float64), canv)
    out = _placed(torch.zeros(Q, S, 4, dtype=torch.float64), canv)
    for t in (kp, sh, ws, out):
        assert t.data_ptr() % 512 == t.element_size()
    check(_lib.lib().rohm_sync_pair_sweep(ptr(kp), ptr(cams), ptr(pairs), ptr(E), ptr(sh), V, N, J, Q, S, 0.2, 4.0, 4.0, ptr(ws), ptr(out),
                                          stream_ptr(torch.device(DEV))), 'rohm_sync_pair_sweep')
    torch.cuda.synchronize()
    assert SM.first_difference(out, want) is None
    _canaries_intact(canv, outputs=(5, 6))
    canv = []
    kp = _placed(torch.from_numpy(np.array(rs['keypoints'])), canv)
    shv = _placed(torch.from_numpy(np.array(rs['shifts'])), canv)
    res = _placed(torch.zeros(V, N, J, 3, dtype=torch.float32), canv)
    check(_lib.lib().rohm_sync_resample(ptr(kp), ptr(shv), V, N, J, ptr(res), stream_ptr(torch.device(DEV))), 'rohm_sync_resample')
    torch.cuda.synchronize()
    assert SM.first_difference(res, want_rs) is None
    _canaries_intact(canv, outputs=(2,))


# ---- graph replay ---------------------------------------------------------------------------------------------------------------------
def test_both_entry_points_record_into_one_graph_and_replay_on_rewritten_inputs():
    """One linear capture on a side stream: the sweep, then the resampler.  A capture that succeeds shows that the calls neither wait
    nor allocate; the replay reads the device operands anew."""
    from rohm_amd import _lib, sync
    from rohm_amd._lib import check, ptr
    first, second = SR.build_sweep_case('many_points'), SR.build_sweep_case('sixteen_views')
    V, N, J = first['keypoints'].shape[:3]
    Q, S = first['shifts'].shape
    # the second value set: other keypoints of the same shape (the sixteen-views case's, tiled), the shifts reversed, the pairs too
    kp2 = np.resize(np.array(second['keypoints']), first['keypoints'].shape).astype(np.float32)
    sets = [dict(kp=first['keypoints'], cams=first['cams'], pairs=first['pairs'], E=first['E'], sh=first['shifts'], rs=SR.build_resample_case('many_points')['shifts']),
            dict(kp=kp2, cams=first['cams'][::-1], pairs=first['pairs'][::-1], E=first['E'][::-1], sh=first['shifts'][:, ::-1],
                 rs=SR.build_resample_case('many_points')['shifts'][::-1])]
    plain = []
    for s in sets:
        plain.append([('sweep', sync.pair_sweep(_dev(s['kp']), _dev(s['cams']), _dev(s['pairs']), _dev(s['E']), _dev(s['sh']))),
                      ('resample', sync.resample_views(_dev(s['kp']), _dev(s['rs'])))])
    torch.cuda.synchronize()
    assert SM.differences(plain[0], plain[1])                              # the two sets can tell a stale input
    slot = {k: _dev(v) for k, v in sets[0].items()}
    ws = torch.empty(sync.ws_bytes(V, N * J) // 8, dtype=torch.float64, device=DEV)
    out, res = torch.empty(Q, S, 4, dtype=torch.float64, device=DEV), torch.empty(V, N, J, 3, dtype=torch.float32, device=DEV)
    side = torch.cuda.Stream(device=DEV)

    def both():
        st = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
        check(_lib.lib().rohm_sync_pair_sweep(ptr(slot['kp']), ptr(slot['cams']), ptr(slot['pairs']), ptr(slot['E']), ptr(slot['sh']), V, N, J, Q, S,
                                              0.2, 4.0, 4.0, ptr(ws), ptr(out), st), 'rohm_sync_pair_sweep')
        check(_lib.lib().rohm_sync_resample(ptr(slot['kp']), ptr(slot['rs']), V, N, J, ptr(res), st), 'rohm_sync_resample')
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both()                                                             # the warm-up
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        both()
    for k in (1, 0, 1):
        for name, v in sets[k].items():
            slot[name].copy_(_dev(v))
        for t in (ws, out, res):
            SM.fill_bytes(t, SM.PATTERNS['ones'])
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert not SM.differences([('sweep', out), ('resample', res)], plain[k]), k


def test_wrappers_refuse_bad_arguments():
    from rohm_amd import sync
    from rohm_amd._lib import RohmHipError
    case = SR.build_sweep_case('many_points')
    kp, cams, pairs, E, sh = (_dev(case[k]) for k in ('keypoints', 'cams', 'pairs', 'E', 'shifts'))
    with pytest.raises(ValueError, match='cams must be'):
        sync.pair_sweep(kp, cams[:2], pairs, E, sh)
    with pytest.raises(ValueError, match='E must be'):
        sync.pair_sweep(kp, cams, pairs, E[:2], sh)
    with pytest.raises(ValueError, match='shifts must be'):
        sync.pair_sweep(kp, cams, pairs, E, sh[:2])
    with pytest.raises(ValueError, match='shifts must be'):
        sync.resample_views(kp, sh[0, :3])
    with pytest.raises(RohmHipError, match='tau_px'):
        sync.pair_sweep(kp, cams, pairs, E, sh, tau_px=0.0)
    with pytest.raises(RohmHipError, match='no CPU fallback'):
        sync.resample_views(kp.cpu(), torch.zeros(4, dtype=torch.float64))
    assert sync.pair_sweep(kp, cams, pairs[:0], E[:0], sh[:0]).shape == (0, 33, 4)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def test_cli_from_unsynchronised_detections_to_a_calibrated_rig(tmp_path, capsys):
    from rohm_amd import multiview, rig, sync
    c = SR.END_TO_END
    K, W, D, kp = SR.make_scene(c['V'], c['N'], c['J'], c['seed'], c['offsets'], c['noise_px'])
    base = dict(keypoints_2d=kp, camera_mtx=K, dist_coeffs=D, fps=SR.FPS, recording_name=np.array('walk'))
    common = ['--max_offset_s', repr(c['max_offset_s']), '--hypotheses', str(c['hypotheses']), '--rounds', str(c['rounds']), '--device', DEV]
    outs = {}
    for key, extra in (('calibrated', {'world2cam': W}), ('uncalibrated', {})):
        src, out, js = (str(tmp_path / f'{key}_{n}') for n in ('raw.npz', 'synced.npz', 'report.json'))
        np.savez(src, **base, **extra)
        assert sync.main(['--views', src, '--out', out, '--json', js] + common) == 0
        text = capsys.readouterr().out
        assert '3 views of 40 frames synchronised' in text and 'wrote' in text
        with open(js) as f:
            rep = json.load(f)['report']
        e = np.abs(np.array(rep['offsets_frames']) - np.array(c['offsets'])).max()
        print(f'end to end, {key}: offsets {np.round(rep["offsets_frames"], 4).tolist()} frames, worst error {e:.4f} (bar {SR.END_TO_END_BARS[key]})')
        record('gpu', f'end_to_end_{key}_offset_frames', e)
        assert rep['calibrated'] == (key == 'calibrated') and [p['coarse_shift'] for p in rep['pairs']] == [-1.0, 3.0, 4.0]
        assert all(p['usable'] for p in rep['pairs']) and e <= SR.END_TO_END_BARS[key]
        with np.load(out, allow_pickle=False) as f:
            outs[key] = {k: f[k] for k in f.files}
        assert sorted(outs[key]) == sorted(dict(base, **extra))            # no key added
        multiview.read_views(outs[key] if extra else dict(outs[key], world2cam=W))                 # a views file as it stands
        assert np.array_equal(outs[key]['keypoints_2d'][0].view(np.uint32), kp[0].view(np.uint32))
    bar_rot, bar_ctr = max(b[0] for b in RR.RECOVERY_BARS.values()), max(b[1] for b in RR.RECOVERY_BARS.values())

    def calibrated_rig(name):
        views, js = str(tmp_path / f'{name}_views.npz'), str(tmp_path / f'{name}_rig.json')
        try:
            rig.main(['--views', str(tmp_path / name), '--out', views, '--json', js, '--hypotheses', '64', '--iters', '10', '--device', DEV])
        except SystemExit as e:                                            # the tool refuses: no rig at all
            return None, str(e)
        with open(js) as f:
            nb = json.load(f)['report']['neighbour']
        return RR.rig_errors(multiview.read_views(views)['world2cam'], W, 0, nb), ''
    got, why = calibrated_rig('uncalibrated_synced.npz')
    assert got is not None, why
    print(f'rig on the synchronised views: rotation {got[0]:.3f} deg (bar {bar_rot}), centre {1e3 * got[1]:.1f} mm (bar {1e3 * bar_ctr:.0f})')
    record('gpu', 'end_to_end_rig_rotation_deg', got[0])
    record('gpu', 'end_to_end_rig_centre_m', got[1])
    assert got[0] <= bar_rot and got[1] <= bar_ctr
    raw, why = calibrated_rig('uncalibrated_raw.npz')
    print('rig on the raw views: ' + (f'rotation {raw[0]:.3f} deg, centre {1e3 * raw[1]:.1f} mm' if raw else f'refused ({why[-120:]})'))
    assert raw is None or raw[0] > bar_rot or raw[1] > bar_ctr             # without sync the same input misses them
