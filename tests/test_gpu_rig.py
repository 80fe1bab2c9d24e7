"""GPU: rig calibration -- `rohm_rig_pair_hypotheses`, `rohm_rig_pair_moments`, `rohm_rig_ba_moments` and `rohm_rig_ba_update`
(csrc/rig.hip) against their float64 restatement (tests/rig_ref.py, held to closed forms, central differences, a dense Jacobian and
planted rigs in tests/test_rig_ref.py), and `python -m rohm_amd.rig` -> `multiview.triangulate_views` end to end.

Shapes.  The pair kernels (`rig_ref.PAIR_CASES`): (V, N, J, Q, K) = (2, 1, 22, 1, 3), one pair, fewer hypotheses than a workgroup
holds; (3, 5, 22, 3, 40), two workgroups per pair, the second ragged; (16, 2, 22, 120, 5), every pair of 16 views; (4, 70, 25, 6, 33),
1 750 points: four LDS tiles, the last ragged.  Salted keypoints (NaN and infinite coordinates, zero, negative and NaN confidences),
one planted outlier per point, and degenerate samples of every clause: an index outside [0, N J), a repeated index, a point one
view does not see, eight times the same point (lambda_2 = 0), a pair outside [0, V), a pair with v1 = v2.  Bundle adjustment
(`rig_ref.BA_CASES`): (V, P) = (2, 22), (3, 110), (16, 44), (4, 1750) -- 110 workgroups, the last with 6 of its 16 points -- and
(3, 4400), 275 tiles: two per workgroup; NaN and infinite points, unobserved entries, points with fewer than two views; sigma_px 0
and 10; lambda 1e-3 and 1e2.

Bars.  Kernel and restatement are both float64 on the same float32 inputs.  E: 1e-9 (a unit vector) where the restatement's
margins hold -- eigen-gap lambda_2 / lambda_9 >= 1e-6, under which cyclic Jacobi and LAPACK agree to 1e-16 / 1e-6; the two largest
|E_i| 1e-9 apart, or the sign rule may turn E over.  Counts, `best` and the NaN / -1 pattern are EQUAL; that rests on no |d - tau_px|
< 1e-6 px, which tests/test_rig_ref.py::test_margins_of_the_gpu_inputs asserts on the CPU for every hypothesis and `_margins`
asserts here once per session.  Moments, S, r, E and the points: 1e-9 relative to the operand's largest magnitude.  The inlier and
observation counts are equal.  The largest measured values go to profiles/rig_parity.json."""
import json

import numpy as np
import pytest
import torch

import multiview_ref as MR
import rig_ref as RR
import stale_memory as SM

record = RR.record
pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BAR = 1e-9
_BA_REF = {}


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)            # a copy: the shared inputs are read-only


@pytest.fixture(scope='session')
def _margins():
    for name in RR.PAIR_CASES:
        case = RR.build_pair_case(name)
        ref = case['ref']
        live = ref['counts'][..., 0] >= 0
        assert (ref['margin_tau'][live] >= 1e-6).all() and (case['margin_moments'] >= 1e-6).all(), name
        assert 1.0 - RR.margins_ok(ref).sum() / live.sum() <= 0.05, name


def hypotheses(case):
    from rohm_amd import rig
    out = rig.pair_hypotheses(_dev(case['keypoints']), _dev(case['cams']), _dev(case['pairs']), _dev(case['samples']))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('name', list(RR.PAIR_CASES))
def test_pair_hypotheses_match_the_restatement(name, _margins):
    case = RR.build_pair_case(name)
    ref = case['ref']
    E, counts, best = (t.cpu().numpy() for t in hypotheses(case))
    assert E.dtype == np.float64 and counts.dtype == np.int64 and best.dtype == np.int32
    live = ref['counts'][..., 0] >= 0
    assert live.any() and (~live).any()
    assert np.array_equal(np.isnan(E), np.isnan(ref['E'])) and np.array_equal(np.isnan(E).all(-1), ~live)      # the NaN / -1 pattern
    ok = RR.margins_ok(ref)
    d = np.abs(E[ok] - ref['E'][ok]).max()
    dc = np.abs(counts - ref['counts']).max()
    print(f'{name}: E {d:.3e} over {int(ok.sum())} of {int(live.sum())} live hypotheses, counts differ by at most {dc}, best {best.tolist()[:8]}')
    record('gpu', 'E_abs', d)
    assert d <= BAR
    assert np.array_equal(counts, ref['counts'])
    assert np.array_equal(best, ref['best'])


@pytest.mark.parametrize('name', list(RR.PAIR_CASES))
def test_pair_moments_match_the_restatement(name, _margins):
    from rohm_amd import rig
    case = RR.build_pair_case(name)
    got = rig.pair_moments(_dev(case['keypoints']), _dev(case['cams']), _dev(case['pairs']), _dev(case['E_best'])).cpu().numpy()
    want = case['ref_moments']
    assert got.shape == want.shape == (len(case['pairs']), 47)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    rows = np.isfinite(want).all(-1)
    assert rows.any() and np.array_equal(got[rows][:, 0], want[rows][:, 0]) and (want[rows][:, 0] >= 8).any()
    d = (np.abs(got[rows] - want[rows]).max(-1) / np.maximum(np.abs(want[rows]).max(-1), 1.0)).max()
    print(f'{name}: moments {d:.3e} relative; inliers {want[rows][:, 0].astype(int).tolist()[:8]}')
    record('gpu', 'moments_rel', d)
    assert d <= BAR
    # the refit of the kernel's sums is the refit of the restatement's
    for q in np.flatnonzero(rows):
        a, b = rig.refit_from_moments(got[q]), RR.refit(want[q])
        assert (a is None) == (b is None)
        if a is not None and np.linalg.eigvalsh(_moment_matrix(want[q]))[1] >= 1e-6 * want[q, 0]:
            assert np.abs(a - b).max() <= 1e-8


def _moment_matrix(m):
    M = np.zeros((9, 9))
    for k, (i, j) in enumerate(RR.TRI):
        M[i, j] = M[j, i] = m[2 + k]
    return M


def ba_reference(name, sigma_px, lam):
    key = (name, sigma_px, lam)
    if key not in _BA_REF:
        case = RR.build_ba_case(name)
        m = RR.ba_moments(case['keypoints'], case['cams'], case['points'], sigma_px=sigma_px, lam=lam)
        X, c = RR.ba_update(case['keypoints'], case['cams'], case['points'], case['dc'], sigma_px=sigma_px, lam=lam)
        _BA_REF[key] = (m, X, c)
    return _BA_REF[key]


@pytest.mark.parametrize('lam', [1e-3, 1e2])
@pytest.mark.parametrize('sigma_px', [0.0, 10.0])
@pytest.mark.parametrize('name', list(RR.BA_CASES))
def test_ba_moments_and_update_match_the_restatement(name, sigma_px, lam):
    from rohm_amd import rig
    case = RR.build_ba_case(name)
    m, X, c = ba_reference(name, sigma_px, lam)
    kp, cams, pts = _dev(case['keypoints']), _dev(case['cams']), _dev(case['points'])
    S, r, stats = (t.cpu().numpy() for t in rig.ba_moments(kp, cams, pts, sigma_px=sigma_px, lam=lam))
    Xn, cn = (t.cpu().numpy() for t in rig.ba_update(kp, cams, pts, _dev(case['dc']), sigma_px=sigma_px, lam=lam))
    V = cams.shape[0]
    assert S.shape == (6 * V, 6 * V) and np.array_equal(S, S.T)
    assert np.isfinite(m['E']) and stats[1] == m['n_obs'] > 0
    dS = np.abs(S - m['S']).max() / np.abs(m['S']).max()
    dr = np.abs(r - m['r']).max() / np.abs(m['r']).max()
    dE = abs(stats[0] - m['E']) / m['E']
    inside = RR.ba_problem(case['keypoints'], case['cams'], case['points'])[3]
    assert inside.any() and (~inside).any()
    assert np.array_equal(Xn[~inside].view(np.uint64), np.array(case['points'])[~inside].view(np.uint64))     # passes through as given
    dX = (np.abs(Xn[inside] - X[inside]).max(-1) / np.maximum(1.0, np.linalg.norm(X[inside], axis=-1))).max()
    dcam = np.abs(cn - c).max()
    print(f'{name} sigma {sigma_px} lambda {lam}: S {dS:.3e}, r {dr:.3e}, E {dE:.3e} relative; points {dX:.3e} m, cams {dcam:.3e}; '
          f'{int(inside.sum())} of {inside.size} points inside, {int(stats[1])} observations')
    for k, v in (('S_rel', dS), ('r_rel', dr), ('E_rel', dE), ('points_m', dX), ('cams_abs', dcam)):
        record('gpu', k, v)
    assert max(dS, dr, dE, dX) <= BAR and dcam <= 1e-12 * np.abs(c).max()
    assert np.array_equal(cn[:, 12:], np.array(case['cams'])[:, 12:])


def test_a_point_behind_a_camera_gives_an_infinite_energy():
    from rohm_amd import rig
    case = RR.build_ba_case('many_points')
    X = np.array(case['points'])
    p = int(np.flatnonzero(RR.ba_problem(case['keypoints'], case['cams'], X)[3])[-1])
    C = -case['cams'][0, :9].reshape(3, 3).T @ case['cams'][0, 9:12]
    X[p] = C - case['cams'][0, 6:9]                                        # a metre behind camera 0
    want = RR.ba_moments(case['keypoints'], case['cams'], X)
    assert want['E'] == np.inf
    S, r, stats = (t.cpu().numpy() for t in rig.ba_moments(_dev(case['keypoints']), _dev(case['cams']), _dev(X)))
    assert stats[0] == np.inf and stats[1] == want['n_obs']
    assert np.abs(S - want['S']).max() <= BAR * np.abs(want['S']).max() and np.abs(r - want['r']).max() <= BAR * np.abs(want['r']).max()


def everything(pattern=None):
    """Every kernel on the many-points cases -> [(label, bytes)]; under `pattern` the outputs and workspaces are poisoned first."""
    import contextlib
    from rohm_amd import rig
    pc, bc = RR.build_pair_case('many_points'), RR.build_ba_case('many_tiles')
    with (SM.poison(pattern) if pattern is not None else contextlib.nullcontext()):
        E, counts, best = rig.pair_hypotheses(_dev(pc['keypoints']), _dev(pc['cams']), _dev(pc['pairs']), _dev(pc['samples']))
        mom = rig.pair_moments(_dev(pc['keypoints']), _dev(pc['cams']), _dev(pc['pairs']), _dev(pc['E_best']))
        S, r, stats = rig.ba_moments(_dev(bc['keypoints']), _dev(bc['cams']), _dev(bc['points']))
        Xn, cn = rig.ba_update(_dev(bc['keypoints']), _dev(bc['cams']), _dev(bc['points']), _dev(bc['dc']))
        torch.cuda.synchronize()
    return [(k, t.cpu().numpy().view(np.uint8)) for k, t in (('E', E), ('counts', counts), ('best', best), ('moments', mom), ('S', S), ('r', r),
                                                              ('stats', stats), ('points_new', Xn), ('cams_new', cn))]


def test_the_same_bits_twice_and_over_poisoned_memory():
    first = everything()
    for pattern in [None] + list(SM.PATTERNS.values()):
        for (k, a), (_, b) in zip(first, everything(pattern)):
            assert np.array_equal(a, b), (k, pattern)


def test_the_contract_case_matches_the_restatement():
    """The inputs of `rig[...]` (tests/header_cases.py), which the four contract families only compare with themselves bit for bit,
    held to the restatement with this module's bars and margins."""
    import header_cases as HC
    i = HC.rig_inputs(7)
    out = {k: v.cpu().numpy() for k, v in HC.rig_call(HC.tensors(HC.rig_inputs, 7, lambda t: t.to(DEV)))}
    ref = RR.pair_hypotheses(i['kp'], i['cams'], i['pairs'], i['samples'])
    live = ref['counts'][..., 0] >= 0
    assert live.any() and (~live).any() and (ref['margin_tau'][live] >= 1e-6).all()
    assert np.array_equal(out['counts'], ref['counts']) and np.array_equal(out['best'], ref['best'])
    ok = RR.margins_ok(ref)
    assert ok.sum() >= 0.95 * live.sum() and np.abs(out['E_all'][ok] - ref['E'][ok]).max() <= BAR
    m = RR.ba_moments(i['kp'], i['cams'], i['points'])
    assert np.abs(out['S'] - m['S']).max() <= BAR * np.abs(m['S']).max() and out['stats'][1] == m['n_obs']


def test_ba_update_without_cams_new_computes_no_cameras_and_keeps_the_points():
    """`cams_new` NULL is not computed, and nothing else changes: `points_new`, one element past a 512-byte boundary between guard
    bands, keeps every bit of the call that had `cams_new`."""
    import guarded_memory as GM
    import header_cases as HC
    from rohm_amd import _lib, rig
    from rohm_amd._lib import check, ptr, stream_ptr
    t = HC.tensors(HC.rig_inputs, 7, lambda t: t.to(DEV))
    canv = []
    Xn = GM.place(torch.zeros(HC.RIG_P, 3, dtype=torch.float64), 'offset', device=DEV, into=canv)
    cn = torch.empty(HC.RIG_V, 24, dtype=torch.float64, device=DEV)
    for cams_new in (cn, None):
        check(_lib.lib().rohm_rig_ba_update(ptr(t['kp']), ptr(t['cams']), ptr(t['points']), ptr(t['dc']), HC.RIG_V, HC.RIG_N, HC.RIG_J, 0.2, 10.0,
                                            1e-3, ptr(Xn), ptr(cams_new), stream_ptr(torch.device(DEV))), 'rohm_rig_ba_update')
        torch.cuda.synchronize()
        if cams_new is not None:
            want = rig.ba_update(t['kp'], t['cams'], t['points'], t['dc'])
            assert SM.first_difference(Xn, want[0]) is None and SM.first_difference(cn, want[1]) is None
            before = canv[0].flat.clone()
    assert torch.equal(canv[0].flat, before)


def test_wrappers_refuse_bad_arguments():
    from rohm_amd import rig
    from rohm_amd._lib import RohmHipError
    case = RR.build_pair_case('three_views')
    kp, cams, pairs, samples = _dev(case['keypoints']), _dev(case['cams']), _dev(case['pairs']), _dev(case['samples'])
    with pytest.raises(ValueError, match='cams must be'):
        rig.pair_hypotheses(kp, cams[:2], pairs, samples)
    with pytest.raises(ValueError, match='samples must be'):
        rig.pair_hypotheses(kp, cams, pairs, samples[:2])
    with pytest.raises(ValueError, match='pairs must be'):
        rig.pair_moments(kp, cams, pairs.reshape(-1), _dev(case['E_best']))
    with pytest.raises(ValueError, match='E must be'):
        rig.pair_moments(kp, cams, pairs, _dev(case['E_best'])[:2])
    with pytest.raises(ValueError, match='points must be'):
        rig.ba_moments(kp, cams, torch.zeros(7, 3, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError, match='dc must be'):
        rig.ba_update(kp, cams, torch.zeros(110, 3, device=DEV, dtype=torch.float64), torch.zeros(2, 6, device=DEV, dtype=torch.float64))
    with pytest.raises(RohmHipError, match='tau_px'):
        rig.pair_hypotheses(kp, cams, pairs, samples, tau_px=-1.0)
    with pytest.raises(RohmHipError, match='lambda'):
        rig.ba_moments(kp, cams, torch.zeros(110, 3, device=DEV, dtype=torch.float64), lam=-1.0)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def test_cli_from_bare_detections_to_a_calibrated_rig(tmp_path, capsys):
    """V = 4, N = 12 (264 points), 2 px of noise, K = 64, 10 iterations: `python -m rohm_amd.rig` recovers the planted rig within the
    bars of tests/test_rig_ref.py (its widest: 264 points are a fifth of its smallest four-view case), and its output through
    `multiview.triangulate_views` gives the planted points within 3 x 2 px x the median sigma_m that call reports.  The scene's seed
    was chosen with the restatement on the CPU: of the seeds 601 to 604, 601 and 602 exceed a bar (centre 10.0 and 13.3 mm against 8;
    worst point 30.6 and 25.2 mm against 25.2), 603 (5.5 mm, 17.9 mm) and 604 (6.9 mm, 19.1 mm) do not."""
    from rohm_amd import multiview, rig
    K, W, D, kp, X = RR.make_scene(4, 12, 22, 603, 2.0, 0.0)
    src, out, js = str(tmp_path / 'uncalibrated.npz'), str(tmp_path / 'views.npz'), str(tmp_path / 'report.json')
    np.savez(src, keypoints_2d=kp, camera_mtx=K, dist_coeffs=D, fps=30.0, recording_name=np.array('rig'))
    assert rig.main(['--views', src, '--out', out, '--json', js, '--hypotheses', '64', '--iters', '10', '--device', DEV]) == 0
    text = capsys.readouterr().out
    assert 'a rig of 4 views calibrated from 12 frames' in text and 'tree from view 0' in text and 'wrote' in text
    with open(js) as f:
        rep = json.load(f)['report']
    assert rep['iterations'] >= 1 and all(a >= b for a, b in zip(rep['energy'], rep['energy'][1:])) and len(rep['pairs']) == 6
    v = multiview.read_views(out)                                          # the output is a views file as it stands
    w2c, nb = v['world2cam'], rep['neighbour']
    rot, ctr = RR.rig_errors(w2c, W, 0, nb)
    bar_rot, bar_ctr = max(b[0] for b in RR.RECOVERY_BARS.values()), max(b[1] for b in RR.RECOVERY_BARS.values())
    print(f'end to end: rotation {rot:.3f} deg (bar {bar_rot}), centre {1e3 * ctr:.1f} mm (bar {1e3 * bar_ctr:.0f}), {rep["iterations"]} iterations, '
          f'median residual {rep["median_residual_px"]:.2f} px')
    record('gpu', 'end_to_end_rotation_deg', rot)
    record('gpu', 'end_to_end_centre_m', ctr)
    assert rot <= bar_rot and ctr <= bar_ctr
    # the scale from the true baseline to the first tree neighbour, then the planted points in the reference camera's frame
    rel = W @ np.linalg.inv(W[0])[None]
    with np.load(out, allow_pickle=False) as f:
        views = {k: f[k] for k in f.files}
    views['world2cam'] = views['world2cam'].copy()
    views['world2cam'][:, :3, 3] *= np.linalg.norm(rel[nb, :3, 3]) / np.linalg.norm(w2c[nb, :3, :3].T @ w2c[nb, :3, 3])
    skeleton, summary = multiview.triangulate_views(views, device=DEV)
    err = np.linalg.norm(skeleton['joints_3d'].astype(np.float64) - (X @ W[0, :3, :3].T + W[0, :3, 3]), axis=-1)
    bar = 3.0 * 2.0 * summary['median_sigma_m']
    print(f'end to end: worst point {1e3 * np.nanmax(err):.1f} mm (bar {1e3 * bar:.1f}), {summary["triangulated"]} of 264 triangulated')
    record('gpu', 'end_to_end_worst_point_m', np.nanmax(err))
    assert summary['triangulated'] == 264 and np.isfinite(err).all() and err.max() <= bar
