"""CPU: the restatement of the synchronisation kernels (tests/sync_ref.py) held to tests/rig_ref.py and to closed forms, and the host
logic of `rohm_amd.sync` on that restatement: planted offsets recovered, `solve_offsets`, the views file, the provisional ABI table,
and the margins on which the equalities of tests/test_gpu_sync.py rest.

Recovery bars.  (V, N) = (3, 90) and (4, 150), J = 22, a smooth walker, planted offsets up to 8 frames, the tool's defaults with
max_offset_s = 0.5; calibrated and uncalibrated, noise-free and with 2 px of noise.  The worst pair-shift and offset errors measured
with the restatement are in profiles/sync_parity.json (group `recovery`); `sync_ref.RECOVERY_BARS` are twice those, as
`rig_ref.RECOVERY_BARS` were made, so that the noise hits only the 2 px cases.  Measured (frames, pair shift / offset): calibrated
8.8e-4 / 3.6e-4 noise-free and 0.112 / 0.083 at 2 px; uncalibrated 0.082 / 0.063 noise-free (three alternations have not converged:
six bring the N = 40 end-to-end case from 0.04 to 0.01) and 0.179 / 0.107 at 2 px.  Independent of the measurement: every coarse shift
is the planted shift rounded to the nearest frame, and the synchronised keypoints triangulate with a smaller median residual than
the raw ones.  The planted pair shifts keep 0.2 frame from a half-integer, where the two nearest frames tie by construction; the
first draft's (0, 3.37, -4.6) and (0, -2.25, 8, 5.55) did not (pair shifts 0.13 and 0.05 from a half) and were replaced before any
bar was set."""
import ctypes
import os

import numpy as np
import pytest
import torch

import multiview_ref as MR
import rig_ref as RR
import stale_memory as SM
import sync_ref as SR

record = SR.record
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restated sweep ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def scene():
    from rohm_amd import sync
    from rohm_amd.multiview import pack_cameras
    K, W, D, kp = SR.make_scene(3, 12, 22, 750, (0.0, 0.0, 0.0), noise_px=1.0)
    kp = MR.salt(kp, 751)
    kp[1:, 1, :, 2] = 0.9
    cams = pack_cameras(K, np.broadcast_to(np.eye(4), (3, 4, 4)), D)
    pairs = np.stack(np.triu_indices(3, 1), 1).astype(np.int32)
    E = np.stack([sync.essential(W, a, b) for a, b in pairs])
    return kp, cams, pairs, E, W, K, D


def test_essential_annihilates_the_two_images_of_a_point():
    from rohm_amd import sync
    from rohm_amd.multiview import pack_cameras
    K, W, D = MR.make_rig(4, 760, False)
    cams = pack_cameras(K, W, D)
    X = np.array([0.0, 0.0, 1.0]) + np.random.Generator(np.random.PCG64(1)).uniform(-1, 1, (50, 3))
    xc = np.einsum('vij,pj->vpi', cams[:, :9].reshape(-1, 3, 3), X) + cams[:, None, 9:12]
    h = xc / xc[..., 2:]
    for a, b in ((0, 1), (2, 0), (1, 3)):
        E = sync.essential(W, a, b).reshape(3, 3)
        assert abs(np.linalg.norm(E) - 1.0) < 1e-14 and np.abs(np.einsum('pi,ij,pj->p', h[b], E, h[a])).max() < 1e-13
    W[1] = W[0]
    assert sync.essential(W, 0, 1) is None


@pytest.mark.parametrize('shift', [0, 1, -2, 5, -11, 11, 12, -12])
def test_sweep_at_an_integer_shift_is_pair_moments_on_the_overlap(scene, shift):
    """The count and sum d^2 of `rig_ref.pair_moments` on the two views sliced to the overlap, bit for bit: the same numpy
    operations on the same operands in the same order."""
    kp, cams, pairs, E, *_ = scene
    N = kp.shape[1]
    out = SR.pair_sweep(kp, cams, pairs, E, np.full((3, 1), float(shift)))[:, 0]
    lo, hi = max(0, -shift), min(N, N - shift)
    for q, (v1, v2) in enumerate(pairs):
        if hi <= lo:
            assert np.array_equal(out[q], np.zeros(4))
            continue
        two = np.stack([kp[v1, lo:hi], kp[v2, lo + shift:hi + shift]])
        m = RR.pair_moments(two, cams[[v1, v2]], [(0, 1)], E[q:q + 1])[0]
        ab = RR.undistorted(two, cams[[v1, v2]])
        assert out[q, 0] == (np.isfinite(ab[0]).all(-1) & np.isfinite(ab[1]).all(-1)).sum()
        assert out[q, 1] == m[0] and out[q, 3] == m[1]
        assert 0 < out[q, 2] <= out[q, 0]
    assert abs(shift) >= N or out[:, 1].max() > 0


def test_sweep_brackets_clause_by_clause(scene):
    kp, cams, pairs, E, *_ = scene
    kp = kp.copy()
    N, J = kp.shape[1:3]
    kp[1] = np.where(np.isfinite(kp[1]), kp[1], 500.0)
    kp[1, :, :, 2] = 0.9                                                   # view 1 sees everything ...
    kp[0, :, :, 2] = 0.0
    kp[0, 0, :, :] = (400.0, 300.0, 0.9)                                   # ... view 0 only frame 0
    pr, Eq = pairs[:1], E[:1]                                              # the pair (0, 1)

    def common(s, k=kp):
        return SR.pair_sweep(k, cams, pr, Eq, np.array([[s]]))[0, 0, 0]
    assert common(float(N - 1)) == J                                       # alpha == 0 at the last frame is common
    assert common(N - 1.5) == J and common(N - 0.5) == 0                   # a fractional shift there is not: i0 + 1 does not exist
    assert common(float(N)) == 0 and common(-1.0) == 0 and common(-0.5) == 0
    hidden = kp.copy()
    hidden[1, 4, 3, 2] = 0.0                                               # an unobserved bracket removes the point
    assert common(3.5, hidden) == J - 1 and common(4.0, hidden) == J - 1 and common(4.5, hidden) == J - 1
    assert common(3.0, hidden) == J and common(5.0, hidden) == J and common(2.5, hidden) == J


def test_sweep_nan_rows_and_zero_rows(scene):
    kp, cams, pairs, E, *_ = scene
    N = kp.shape[1]
    pr = np.array([(0, 1), (0, 3), (2, 2), (-1, 0), (0, 1)], np.int32)
    Eq = np.stack([E[0], E[0], E[0], E[0], np.full(9, np.nan)])
    sh = np.tile(np.array([0.0, 0.5, np.nan, np.inf, float(N), -N - 0.25]), (5, 1))
    out = SR.pair_sweep(kp, cams, pr, Eq, sh)
    assert np.isnan(out[1:4]).all()                                        # outside [0, V), v1 = v2
    assert np.isnan(out[[0, 4]][:, 2:4]).all()                             # a shift that is not finite
    assert np.array_equal(out[[0, 4]][:, 4:], np.zeros((2, 2, 4)))         # nothing is common
    assert (out[0, :2, :2] > 0).all() and np.isfinite(out[0, :2]).all()
    assert (out[4, :2, 0] == out[0, :2, 0]).all() and (out[4, :2, 1] == 0).all() and (out[4, :2, 3] == 0).all()      # E not finite: no inliers
    assert (out[4, :2, 2] == out[4, :2, 0]).all()                          # and every common point at the robust function's supremum
    plain = SR.pair_sweep(kp, cams, pr[:1], Eq[:1], sh[:1, :2], sigma_px=0.0)
    assert (plain[0, :, 2] >= plain[0, :, 3]).all() and plain[0, 1, 2] > plain[0, 1, 3] and plain[0, 1, 1] < plain[0, 1, 0]      # sum d^2 over all against over the inliers


def test_sweep_interpolates_in_normalised_coordinates(scene):
    """At alpha = 1/4 view 2's point is (3 a(i0) + a(i0 + 1)) / 4: the sweep on the pair equals the sweep at shift 0 against a view
    built from those undistorted points (no distortion, unit focal lengths put back through the pair scale)."""
    kp, cams, pairs, E, *_ = scene
    V, N, J = kp.shape[:3]
    ab = RR.undistorted(kp, cams).reshape(V, N, J, 2)
    mixed = 0.75 * ab[1, :-1] + 0.25 * ab[1, 1:]                           # NaN where a bracket is unobserved
    plain = cams[[0, 1]].copy()
    plain[1, 16:21] = 0.0
    k2 = np.zeros((2, N - 1, J, 3))
    k2[0] = kp[0, :-1]
    k2[1, ..., 0], k2[1, ..., 1] = mixed[..., 0] * plain[1, 12] + plain[1, 14], mixed[..., 1] * plain[1, 13] + plain[1, 15]
    k2[1, ..., 2] = np.where(np.isfinite(mixed).all(-1), 0.9, 0.0)
    k2[1] = np.nan_to_num(k2[1])
    want = RR.pair_moments(k2, plain, [(0, 1)], E[:1], as_given=True)[0]
    got = SR.pair_sweep(kp[:, :], cams, pairs[:1], E[:1], np.array([[0.25]]))[0, 0]
    assert got[1] == want[0] > 20 and abs(got[3] - want[1]) <= 1e-9 * want[1]


# ---- the restated resampler ----------------------------------------------------------------------------------------------------------
def test_resampler_clause_by_clause(scene):
    kp = scene[0]
    V, N, J = kp.shape[:3]
    out = SR.resample(kp, [0.0, 3.0, -2.0])
    assert np.array_equal(out[0].view(np.uint32), kp[0].view(np.uint32))                           # zero shift: a bit copy, NaN and all
    assert np.array_equal(out[1, :N - 3].view(np.uint32), kp[1, 3:].view(np.uint32)) and not out[1, N - 3:].any()      # an integer shift: a slice
    assert np.array_equal(out[2, 2:].view(np.uint32), kp[2, :N - 2].view(np.uint32)) and not out[2, :2].any()
    k = np.zeros((1, 4, 3, 3), np.float32)
    k[0, :, :, 0] = np.arange(4)[:, None] * 10.0 + np.arange(3)
    k[0, :, :, 1] = 7.0
    k[0, :, :, 2] = [[0.9, 0.8, 0.7], [0.5, 0.0, np.nan], [0.6, 0.9, 0.9], [0.9, np.inf, -1.0]]
    o = SR.resample(k, [0.25])[0]
    assert np.allclose(o[0], [[2.5, 7.0, 0.5], [1.0, 7.0, 0.0], [2.0, 7.0, 0.0]])                 # min(c0, c1); the confidence-0 bracket rule
    assert np.allclose(o[1], [[12.5, 7.0, 0.5], [21.0, 7.0, 0.0], [22.0, 7.0, 0.0]])              # (x, y) of the other bracket
    assert np.allclose(o[2], [[22.5, 7.0, 0.6], [21.0, 7.0, 0.0], [22.0, 7.0, 0.0]])              # inf and negative confidences have no position
    assert not o[3].any()                                                                          # i0 + 1 outside [0, N): zeros
    k[0, 0, 0] = (np.nan, 1.0, 0.9)
    k[0, 1, 0] = (1.0, 1.0, 0.0)
    assert not SR.resample(k, [0.5])[0, 0, 0].any()                                                # neither bracket has a position
    assert not SR.resample(k, [np.nan]).any() and not SR.resample(k, [4.0]).any() and not SR.resample(k, [-4.0]).any()
    x = SR.resample(kp, [0.3, 0.3, 0.3]).astype(np.float64)
    both = (kp[:, :-1, :, 2] > 0) & (kp[:, 1:, :, 2] > 0) & np.isfinite(kp[:, :-1]).all(-1) & np.isfinite(kp[:, 1:]).all(-1)
    want = 0.7 * kp[:, :-1, :, :2].astype(np.float64) + 0.3 * kp[:, 1:, :, :2].astype(np.float64)
    assert np.abs(x[:, :-1, :, :2][both] - want[both]).max() <= 2.0 ** -24 * np.abs(want[both]).max()      # rounded once to float32


# ---- solve_offsets --------------------------------------------------------------------------------------------------------------------
def test_solve_offsets():
    from rohm_amd import sync
    g = np.random.Generator(np.random.PCG64(5))
    V = 5
    o = np.concatenate([[0.0], g.uniform(-9, 9, V - 1)])
    pairs = np.stack(np.triu_indices(V, 1), 1)
    s = SR.pair_shifts(o, pairs)
    w = g.integers(50, 900, len(pairs)).astype(np.float64)
    got, resid = sync.solve_offsets(pairs, s, w, V)
    assert np.abs(got - o).max() <= 1e-12 and np.abs(resid).max() <= 1e-12 and got[0] == 0.0
    got2, _ = sync.solve_offsets(pairs, s, w, V, ref=3)                   # another reference: the same differences
    assert got2[3] == 0.0 and np.abs((got2 - got2[0]) - o).max() <= 1e-12
    w2 = w.copy()
    w2[(pairs == 4).any(1)] = 0.0                                          # view 4 loses every pair
    with pytest.raises(ValueError, match=r'views \[4\] cannot be chained to view 0'):
        sync.solve_offsets(pairs, s, w2, V)
    w3 = np.where((pairs[:, 0] == 0) | (pairs[:, 1] == 0), 0.0, w)         # the reference loses every pair
    with pytest.raises(ValueError, match=r'views \[1, 2, 3, 4\] cannot be chained to view 0'):
        sync.solve_offsets(pairs, s, w3, V)
    chain = np.array([(0, 1), (1, 2), (2, 3), (3, 4)])                     # a tree: no cycle, no residual
    got3, r3 = sync.solve_offsets(chain, SR.pair_shifts(o, chain), np.ones(4), V)
    assert np.abs(got3 - o).max() <= 1e-12 and np.abs(r3).max() <= 1e-12
    s4 = s.copy()
    s4[0] += 0.6                                                           # the pair (0, 1) disagrees with the cycles through it
    got4, r4 = sync.solve_offsets(pairs, s4, np.ones(len(pairs)), V)
    assert np.argmax(np.abs(r4)) == 0 and 0.3 < r4[0] < 0.6 and abs(r4.sum()) < 1.0 and np.abs(got4 - o).max() < 0.3
    three = np.array([(0, 1), (0, 2), (1, 2)])
    _, r5 = sync.solve_offsets(three, [1.0, 3.0, 2.3], np.ones(3), 3)      # closed form: the cycle's excess 0.3 in equal thirds
    assert np.abs(r5 - np.array([0.1, -0.1, 0.1])).max() <= 1e-12        # s01 + s12 - s02 = 0.3
    assert sync.parabola_vertex(4.0, 1.0, 2.0) == pytest.approx(0.25) and sync.parabola_vertex(1.0, 1.0, 1.0) == 0.0
    assert sync.parabola_vertex(1.0, 2.0, 1.0) == 0.0 and sync.parabola_vertex(np.inf, 1.0, 2.0) == 0.0


# ---- recovery with the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('noise_px', [0.0, 2.0])
@pytest.mark.parametrize('calibrated', [True, False])
@pytest.mark.parametrize('name', list(SR.RECOVERY))
def test_planted_offsets_are_recovered(name, calibrated, noise_px, monkeypatch):
    from rohm_amd import sync
    from rohm_amd.multiview import pack_cameras
    SR.on_reference(monkeypatch)
    V, N, offsets, seed = SR.RECOVERY[name]
    K, W, D, kp = SR.make_scene(V, N, 22, seed, offsets, noise_px)
    synced, rep = sync.synchronise(kp, K, D, SR.FPS, W if calibrated else None, device='cpu', **SR.RECOVERY_OPTIONS)
    pairs = np.array([p['pair'] for p in rep['pairs']])
    want = SR.pair_shifts(offsets, pairs)
    assert np.abs(np.abs(want - np.floor(want)) - 0.5).min() >= 0.2        # no planted shift near the tie between two frames
    got = np.array([p['shift_frames'] for p in rep['pairs']])
    e_pair, e_off = np.abs(got - want).max(), np.abs(np.array(rep['offsets_frames']) - np.array(offsets)).max()
    key = ('calibrated' if calibrated else 'uncalibrated') + ('_2px' if noise_px else '_noise_free')
    print(f'{name} {key}: pair shift {e_pair:.4f}, offset {e_off:.4f} frames; peak ratios {[round(p["peak_ratio"], 1) for p in rep["pairs"]]}')
    record('recovery', key + '_pair_shift_frames', e_pair)
    record('recovery', key + '_offset_frames', e_off)
    assert [p['coarse_shift'] for p in rep['pairs']] == np.round(want).tolist()
    assert all(p['usable'] and len(p['fine_shifts']) == (1 if calibrated else 3) for p in rep['pairs'])
    assert rep['offsets_frames'][0] == 0.0 and np.allclose(np.array(rep['offsets_s']) * SR.FPS, rep['offsets_frames'])
    assert np.allclose([p['cycle_residual_frames'] for p in rep['pairs']], got - SR.pair_shifts(rep['offsets_frames'], pairs))
    assert [r['frames_outside_share'] > 0 for r in rep['per_view']] == [o != 0 for o in offsets]
    bar_pair, bar_off = SR.RECOVERY_BARS[calibrated, noise_px]
    assert e_pair <= bar_pair and e_off <= bar_off
    cams = pack_cameras(K, W, D)
    med = [np.nanmedian(MR.view_residuals(MR.triangulate(k, cams)['joints'], k, cams)) for k in (kp, synced)]
    print(f'    median view residual {med[0]:.2f} px raw, {med[1]:.2f} px synchronised')
    assert med[1] < med[0]


def test_the_end_to_end_case_of_the_gpu_test_with_the_restatement(monkeypatch):
    """The bars of tests/test_gpu_sync.py's end-to-end case: the restatement's own worst offset error on that scene, recorded in
    profiles/sync_parity.json (group `end_to_end_cpu`); the GPU test allows twice that."""
    from rohm_amd import sync
    SR.on_reference(monkeypatch)
    c = SR.END_TO_END
    K, W, D, kp = SR.make_scene(c['V'], c['N'], c['J'], c['seed'], c['offsets'], c['noise_px'])
    for calibrated in (True, False):
        _, rep = sync.synchronise(kp, K, D, SR.FPS, W if calibrated else None, device='cpu', max_offset_s=c['max_offset_s'], hypotheses=c['hypotheses'],
                                  rounds=c['rounds'])
        e = np.abs(np.array(rep['offsets_frames']) - np.array(c['offsets'])).max()
        key = 'calibrated' if calibrated else 'uncalibrated'
        print(f'end to end on the restatement, {key}: offset {e:.4f} frames')
        record('end_to_end_cpu', key + '_offset_frames', e)
        assert e <= SR.END_TO_END_BARS[key]
        assert [p['coarse_shift'] for p in rep['pairs']] == [-1.0, 3.0, 4.0]


# ---- the views file -------------------------------------------------------------------------------------------------------------------
def test_views_file_in_and_out(monkeypatch, tmp_path):
    from rohm_amd import multiview, sync
    SR.on_reference(monkeypatch)
    offsets = (0.0, 2.0, -1.5)
    K, W, D, kp = SR.make_scene(3, 30, 22, 770, offsets)
    base = dict(keypoints_2d=kp, camera_mtx=K, dist_coeffs=D, fps=np.float64(SR.FPS), recording_name=np.array('walk'),
                frame_names=np.array(['f%03d' % n for n in range(30)]))
    opts = dict(device='cpu', max_offset_s=4.0 / SR.FPS, hypotheses=32)
    for extra in ({}, {'world2cam': W}, {'cam2world': np.linalg.inv(W)}):
        src = dict(base, **extra)
        path = str(tmp_path / 'raw.npz')
        np.savez(path, **src)
        out, rep = sync.synchronise_views(path, **opts)
        assert list(out) == [k for k in multiview.VIEW_KEYS if k in src]                           # no key added, none lost
        assert rep['calibrated'] == bool(extra) and np.abs(np.array(rep['offsets_frames']) - offsets).max() < 0.2
        for k in src:
            if k != 'keypoints_2d':
                assert np.array_equal(out[k], src[k])
        assert out['keypoints_2d'].dtype == np.float32 and out['keypoints_2d'].shape == kp.shape
        assert np.array_equal(out['keypoints_2d'][0].view(np.uint32), kp[0].view(np.uint32))       # the reference view keeps its bits
        multiview.read_views(out if extra else dict(out, world2cam=W))                              # a views file as it stands
        want = SR.resample(kp, -np.array(rep['offsets_frames']))
        assert np.array_equal(out['keypoints_2d'].view(np.uint32), want.view(np.uint32))
    times = 5.0 + np.arange(30) / SR.FPS
    src = {k: v for k, v in base.items() if k != 'fps'}
    out, rep = sync.synchronise_views(dict(src, times=times), **opts)
    assert 'fps' not in out and np.array_equal(out['times'], times) and abs(rep['fps'] - SR.FPS) < 1e-9
    bent = times.copy()
    bent[7] += 1e-4 / SR.FPS
    with pytest.raises(ValueError, match='times is not uniform'):
        sync.synchronise_views(dict(src, times=bent), **opts)
    with pytest.raises(ValueError, match=r'the number of views must be in \[2, 16\], got 1'):
        sync.synchronise_views(dict(base, keypoints_2d=kp[:1], camera_mtx=K[:1], dist_coeffs=D[:1]), **opts)
    with pytest.raises(ValueError, match=r"unknown keys \['offsets'\]"):
        sync.synchronise_views(dict(base, offsets=np.zeros(3)), **opts)
    with pytest.raises(ValueError, match='exactly one of fps and times'):
        sync.synchronise_views(dict(base, times=times), **opts)
    with pytest.raises(ValueError, match='ref_view'):
        sync.synchronise_views(base, ref_view=3, **opts)


# ---- the provisional table --------------------------------------------------------------------------------------------------------------
def test_provisional_headers_table_and_library_agree():
    """As tests/test_host_logic.py::test_abi_headers_table_and_library_agree does for `_lib.HEADERS`: the files of include/provisional/,
    `_lib.PROVISIONAL_HEADERS`, `_lib.PROVISIONAL_SIGNATURES` and the built library agree."""
    import stream_order as SO
    from rohm_amd import _lib
    folder = os.path.join(ROOT, 'include', 'provisional')
    assert sorted(_lib.PROVISIONAL_HEADERS) == sorted(f for f in os.listdir(folder) if f.endswith('.h'))
    assert not set(_lib.PROVISIONAL_HEADERS) & set(_lib.HEADERS) and not set(_lib.PROVISIONAL_SIGNATURES) & set(_lib.SIGNATURES)
    names = []
    raw, L = ctypes.CDLL(_lib.LIB_PATH), _lib.lib()
    for h in _lib.PROVISIONAL_HEADERS:
        with open(os.path.join(folder, h)) as f:
            text = f.read()
        for name, params in SM.declarations(text):
            names.append(name)
            assert hasattr(raw, name), f'{name} declared in {h} but not exported'
            res, args = _lib.PROVISIONAL_SIGNATURES[name]
            fn = getattr(L, name)
            assert fn.restype is res and list(fn.argtypes) == list(args), name
            assert len(args) == len(params), f'{name}: {len(params)} parameters in {h}, {len(args)} ctypes arguments'
        assert '#include "../rohm_hip.h"' in text and 'PROVISIONAL' in text
        assert 'obey rohm_hip.h\'s "Conventions" and "Caller-owned memory" word for word' in SO.header_prose(text), h
    assert len(names) == len(set(names)) and set(names) == set(_lib.PROVISIONAL_SIGNATURES)
    assert set(names) == {'rohm_sync_ws_bytes', 'rohm_sync_pair_sweep', 'rohm_sync_resample'}
    assert not set(names) & {n for n, _ in SM.declarations()}                                      # no name is in a public header as well
    assert L.rohm_sync_ws_bytes(4, 1750) == L.rohm_rig_pair_ws_bytes(4, 1750) == 4 * 1750 * 16
    assert L.rohm_sync_ws_bytes(1, 10) < 0 and b'V must be in [2, 16]' in L.rohm_last_error()
    assert L.rohm_sync_ws_bytes(2, (1 << 29) + 1) < 0 and b'P must be in' in L.rohm_last_error()


def test_argument_errors_name_the_argument_before_any_launch():
    """The checks of rohm_sync.h come before the first launch: null pointers and no device are enough to see every one of them."""
    from rohm_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(64)                                                # never dereferenced: every call below fails its checks first

    def sweep(V=2, N=3, J=22, Q=1, S=1, conf=0.2, tau=4.0, sigma=4.0, kp=p, cams=p, pairs=p, E=p, shifts=p, ws=p, out=p):
        rc = L.rohm_sync_pair_sweep(kp, cams, pairs, E, shifts, V, N, J, Q, S, conf, tau, sigma, ws, out, None)
        return rc, L.rohm_last_error().decode()
    for kw, word in ((dict(V=1), 'V must be in [2, 16]'), (dict(V=17), 'V must be'), (dict(N=0), 'N must be'), (dict(J=0), 'J must be'),
                     (dict(N=1 << 15, J=(1 << 14) + 1), 'N * J must not exceed'), (dict(Q=-1), 'Q must be'), (dict(S=0), 'S must be'),
                     (dict(Q=1 << 10, S=(1 << 10) + 1), 'Q * S must not exceed'), (dict(conf=np.nan), 'conf_min'), (dict(tau=0.0), 'tau_px'),
                     (dict(tau=np.inf), 'tau_px'), (dict(sigma=-1.0), 'sigma_px'), (dict(sigma=np.nan), 'sigma_px'), (dict(kp=None), 'keypoints is null'),
                     (dict(cams=None), 'cams is null'), (dict(pairs=None), 'pairs is null'), (dict(E=None), 'E is null'),
                     (dict(shifts=None), 'shifts is null'), (dict(ws=None), 'ws is null'), (dict(out=None), 'out is null')):
        rc, msg = sweep(**kw)
        assert rc < 0 and msg.startswith('sync_pair_sweep: ') and word in msg, (kw, msg)
    assert sweep(Q=0, kp=None, out=None)[0] == 0                           # Q == 0 returns without a launch

    def resample(V=2, N=3, J=22, kp=p, shifts=p, out=p):
        rc = L.rohm_sync_resample(kp, shifts, V, N, J, out, None)
        return rc, L.rohm_last_error().decode()
    for kw, word in ((dict(V=0), 'V must be in [1, 16]'), (dict(V=17), 'V must be'), (dict(N=0), 'N must be'), (dict(J=-1), 'J must be'),
                     (dict(N=1 << 15, J=(1 << 14) + 1), 'N * J must not exceed'), (dict(kp=None), 'keypoints is null'),
                     (dict(shifts=None), 'shifts is null'), (dict(out=None), 'out is null')):
        rc, msg = resample(**kw)
        assert rc < 0 and msg.startswith('sync_resample: ') and word in msg, (kw, msg)


# ---- the margins the GPU equalities rest on -------------------------------------------------------------------------------------------
def test_margins_of_the_gpu_inputs():
    """For every case of tests/test_gpu_sync.py: no common point within 1e-6 px of tau_px, no interpolation index within 1e-9 of an
    integer unless the shift is an integer exactly -- none is left out, a failing seed is replaced in sync_ref.SWEEP_CASES.  And the
    cases hold what their names promise."""
    for name, (V, N, J, Q, S, seed, bad_E) in SR.SWEEP_CASES.items():
        case = SR.build_sweep_case(name)
        ref, sh = case['ref'], case['shifts']
        assert ref.shape == (Q, S, 4) and case['keypoints'].shape == (V, N, J, 3)
        assert (case['margin_tau'] >= 1e-6).all() and (case['margin_index'] >= 1e-9).all(), name
        whole = np.isfinite(sh) & (sh == np.floor(sh))
        assert whole.any() and (np.isfinite(sh) & ~whole).any() and (sh < 0).any() and (np.isnan(sh).sum(1) == 1).all(), name
        assert not np.isfinite(case['keypoints']).all() and np.isfinite(case['E']).all() != bad_E
        live = np.isfinite(ref).all(-1)
        assert np.array_equal(np.isnan(ref).all(-1), ~live) and live.any() and (~live).any()
        assert (ref[live][:, 0] == 0).any() or N > 3 * 9                   # empty overlaps wherever the shifts can reach past the recording
        if name != 'one_pair_E_not_finite':
            assert (ref[live][:, 1] > 0).any() and (ref[live][:, 1] < ref[live][:, 0]).any(), name
        rs = SR.build_resample_case(name)
        assert np.isfinite(rs['shifts']).sum() >= 2 and rs['shifts'][0] == 0.0
