"""GPU parity of the clip builder, the keypoint undistortion and the visibility masks (csrc/clips.hip through
rohm_amd/data_loaders/clips.py) against the reference's own outputs (tests/golden/clips.npz, scripts/make_golden_clips.py)
and against the numpy restatement (tests/clips_ref.py) + the oracle's `get_repr_smplx` (oracle/rederive.py)."""
import functools

import numpy as np
import pytest
import torch

import clips_ref as CR
from helpers import golden
from oracle import rederive as RD
from rohm_amd.utils import synth

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GEOM_TOL = 5e-6                 # dataset-side geometry, as tests/test_gpu_frames.py
LOCAL_FACTOR = 4 * 0.0112       # see _close


def _close(out, ref, cano, std=None, tol=2e-5):
    """The rule of tests/test_gpu_rederive.py::_close on all 294 channels: `tol` absolute, plus the conditioning term of
    the reference's own float32 facing computation, term = 3e-6 / |across_xy| + 4e-6 / w (oracle.rederive.facing_margin),
    on channels 0, 1, 4, 5.  On local_positions / local_vel (channels 22..153: vectors rotated by the facing
    quaternion) the same term applies times LOCAL_FACTOR times the rotated vector's length in metres (at least 1).

    LOCAL_FACTOR: on every input of this file (the four fixture cases, the degenerate clip and the restatement cases,
    normalised where the test normalises) the reference's float32 flow (oracle) was compared on the CPU with the same
    computation in float64 throughout (clips_ref.get_repr_f64); the largest |f32 - f64| / (term * max(len, 1)) over
    channels 22..153 was 0.0112 (tests/test_clips_ref.py::test_local_factor_measurement re-measures it); 4x that.
    Contact channels (290..293) must be exactly equal; `ref` is float64, `out` the device's float32."""
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    lim = CR.repr_limits(ref, cano, std, tol, LOCAL_FACTOR)
    err = np.abs(out - ref)
    assert (err <= lim).all(), f'max err {err.max():.3e}; outside tolerance at {np.argwhere(err > lim)[:5].tolist()}'
    assert np.array_equal(out[..., 290:], ref[..., 290:].astype(np.float32))


@functools.lru_cache(maxsize=None)
def _recording(seed, N, up_axis, degenerate=()):
    return synth.synthetic_recording(seed, N, up_axis, degenerate_frames=degenerate)


def _dev(jw, world):
    return torch.from_numpy(jw).to(DEV), torch.from_numpy(world).to(DEV)


def _build(*a, **k):
    from rohm_amd.data_loaders.clips import build_clips
    return {n: v.cpu().numpy() for n, v in build_clips(*a, **k).items()}


def _check_geometry(out, ref):
    for k in ('cano_joints', 'global_orient', 'transl', 'transf_matrix'):
        assert out[k].dtype == np.float32 and out[k].shape == ref[k].shape, k
        assert np.abs(out[k] - ref[k]).max() <= GEOM_TOL, (k, np.abs(out[k] - ref[k]).max())


@pytest.mark.parametrize('up_axis', ['z', 'y'])
@pytest.mark.parametrize('floor', ['min', 'preset'])
def test_build_clips_vs_reference_golden(up_axis, floor):
    g = golden('clips.npz')
    p = f'{up_axis}_{floor}_'
    N, L, ov = int(g['N']), int(g['L']), int(g['overlap'])
    ref = {k: g[p + k] for k in ('cano_joints', 'global_orient', 'transl', 'transf_matrix', 'repr')}
    # on the reference's side: both contact values occur and no decision is within a relative 1e-3 of a threshold
    assert CR.contact_margin(ref['cano_joints']) > 1e-3
    assert set(np.unique(ref['repr'][..., 290:])) == {0.0, 1.0} and not np.isnan(ref['repr']).any()
    jw, world = _recording(int(g['seed']), N, up_axis)
    preset = float(g[p + 'preset']) if floor == 'preset' else None
    out = _build(*_dev(jw, world), L, ov, up_axis, preset)
    assert out['repr'].shape == (3, L - 1, 294) and out['repr'].dtype == np.float32
    assert out['starts'].tolist() == [0, 14, 28]
    _check_geometry(out, ref)
    _close(out['repr'], ref['repr'], ref['cano_joints'])


CASES = [(145, 145, 2), (300, 145, 2), (40, 2, 0)]


@pytest.mark.parametrize('up_axis', ['z', 'y'])
@pytest.mark.parametrize('N,L,ov', CASES)
def test_build_clips_vs_restatement_shapes(N, L, ov, up_axis):
    jw, world = _recording(21, N, up_axis)
    stats = synth.synthetic_stats(3)
    ref = CR.build_clips(jw, world, L, ov, up_axis)
    assert CR.contact_margin(ref['cano_joints']) > 1e-3
    d = _dev(jw, world)
    out = _build(*d, L, ov, up_axis)
    assert out['repr'].shape == (CR.n_windows(N, L, ov), L - 1, 294)
    _check_geometry(out, ref)
    _close(out['repr'], ref['repr'], ref['cano_joints'])
    norm = _build(*d, L, ov, up_axis, stats=stats)
    _close(norm['repr'], (ref['repr'] - stats[0]) / stats[1], ref['cano_joints'], std=stats[1])
    assert np.array_equal(norm['cano_joints'], out['cano_joints'])


def test_build_clips_zero_clips_is_empty():
    from rohm_amd.data_loaders.clips import build_clips
    jw, world = _recording(21, 10, 'z')
    out = build_clips(*_dev(jw, world), 16, 2)
    assert out['repr'].shape == (0, 15, 294) and out['cano_joints'].shape == (0, 16, 22, 3)
    assert out['global_orient'].shape == (0, 16, 3) and out['transf_matrix'].shape == (0, 4, 4) and out['starts'].shape == (0,)


def test_build_clips_explicit_starts_and_floor_quirk():
    jw, world = _recording(21, 40, 'z')
    d = _dev(jw, world)
    starts = [3, 3, 20]
    ref = CR.build_clips(jw, world, 16, starts=starts)
    for st in (starts, torch.tensor(starts, device=DEV, dtype=torch.int32)):
        out = _build(*d, 16, starts=st)
        assert out['starts'].tolist() == starts
        _check_geometry(out, ref)
        _close(out['repr'], ref['repr'], ref['cano_joints'])
        assert np.array_equal(out['repr'][0], out['repr'][1])           # bitwise reproducible
    # `if preset_floor_height:` -- 0.0 is "not given"
    zero, none = _build(*d, 16, preset_floor_height=0.0), _build(*d, 16)
    for k in none:
        assert np.array_equal(zero[k], none[k]), k
    other = _build(*d, 16, preset_floor_height=CR.clip_preset(jw, 'z'))
    assert np.abs(other['cano_joints'][..., 2] - none['cano_joints'][..., 2]).min() > 0.01


def test_build_clips_long_clips_use_the_scratch_buffer():
    """clip_len 300: the float64 canonical joints of a clip (300 x 66 doubles) no longer fit into LDS."""
    from rohm_amd._lib import lib
    assert lib().rohm_clips_scratch_bytes(3, 145) == 0 and lib().rohm_clips_scratch_bytes(3, 300) == 3 * 300 * 66 * 8
    jw, world = _recording(21, 300, 'z')
    ref = CR.build_clips(jw, world, 300, 2)
    out = _build(*_dev(jw, world), 300, 2)
    _check_geometry(out, ref)
    _close(out['repr'], ref['repr'], ref['cano_joints'])


def test_build_clips_degenerate_facing_reproduces_reference_nan_pattern():
    g = golden('clips.npz')
    ref, cano = g['degenerate_repr'], g['degenerate_cano_joints']
    nan = np.isnan(ref)
    assert nan[0, 9, 0] and not nan[0, :9, 0].any() and nan[0, 8, 1] and nan[0, 9, 1] and nan[0, 8, 4] and nan[0, 9, 22:154].all()
    L = int(g['L'])
    jw, world = _recording(int(g['seed']), L, 'z', tuple(CR.DEGENERATE_FRAMES))
    out = _build(*_dev(jw, world), L)
    assert np.abs(out['cano_joints'] - cano).max() <= GEOM_TOL
    assert np.array_equal(np.isnan(out['repr']), nan)
    with np.errstate(invalid='ignore'):
        _close(np.where(nan, 0.0, out['repr']), np.where(nan, 0.0, ref), np.nan_to_num(cano, nan=0.0))


def _keypoints(seed=0, shape=(3, 8, 22)):
    g = np.random.Generator(np.random.PCG64(seed))
    kp = np.concatenate([g.uniform(size=shape + (2,)) * np.array([1920., 1080.]), g.uniform(size=shape + (1,))], -1)
    kp[0, 0, :4, 2] = [0.2, np.float32(0.2), 0.19999, 0.20001]           # around the confidence threshold
    kp[0, 1] = 0.0                                                       # a frame without people
    return kp.astype(np.float32)


PROX_K, PROX_DIST = CR.PROX_K, CR.PROX_DIST


def test_undistort_keypoints_vs_restatement():
    from rohm_amd.data_loaders.clips import undistort_keypoints
    kp = _keypoints()
    out = undistort_keypoints(torch.from_numpy(kp).to(DEV), PROX_K, PROX_DIST)
    assert out.shape == kp.shape and out.dtype == torch.float32
    ref = CR.undistort_keypoints(kp, PROX_K, PROX_DIST)
    out = out.cpu().numpy()
    assert np.abs(out[..., :2] - ref[..., :2]).max() <= 1e-3            # float32 storage of values up to 1920 (ulp 1.2e-4)
    assert np.array_equal(out[..., 2], kp[..., 2])
    assert np.abs(ref[..., :2] - kp[..., :2]).max() > 1.0               # the distortion is not a no-op here


def test_visibility_masks_vs_restatement():
    from rohm_amd.data_loaders.clips import visibility_masks
    kp = _keypoints()
    g = np.random.Generator(np.random.PCG64(3))
    mask = (g.uniform(size=(3, 8, 25)) > 0.3).astype(np.float32)
    flat_kp, flat_mask = kp.reshape(24, 22, 3), mask.reshape(24, 25)
    jv, vv = visibility_masks(torch.from_numpy(flat_kp).to(DEV), torch.from_numpy(flat_mask).to(DEV), 8, overlap_len=0)
    rj, rv = CR.visibility_masks(kp, mask)
    assert jv.shape == (3, 8, 22) and vv.shape == (3, 8, 294) and jv.dtype == vv.dtype == torch.float32
    assert np.array_equal(jv.cpu().numpy(), rj) and np.array_equal(vv.cpu().numpy(), rv)
    assert 0.2 < rv[..., 290:].mean() < 0.8 and rj[0, 1].sum() == 0
    # overlapping windows and explicit starts read the same frames in place
    jv2, vv2 = visibility_masks(torch.from_numpy(flat_kp).to(DEV), torch.from_numpy(flat_mask).to(DEV), 8, starts=[0, 5, 16])
    rj2, rv2 = CR.visibility_masks(np.stack([flat_kp[s:s + 8] for s in (0, 5, 16)]), np.stack([flat_mask[s:s + 8] for s in (0, 5, 16)]))
    assert np.array_equal(jv2.cpu().numpy(), rj2) and np.array_equal(vv2.cpu().numpy(), rv2)


def test_clips_reject_cpu_tensors_and_bad_shapes():
    from rohm_amd._lib import RohmHipError
    from rohm_amd.data_loaders.clips import build_clips, undistort_keypoints, visibility_masks
    jw, world = _recording(21, 40, 'z')
    tj, tw = torch.from_numpy(jw), torch.from_numpy(world)
    with pytest.raises(RohmHipError):
        build_clips(tj, tw, 16)
    with pytest.raises(RohmHipError):
        undistort_keypoints(torch.zeros(4, 3), PROX_K, PROX_DIST)
    with pytest.raises(RohmHipError):
        visibility_masks(torch.zeros(8, 22, 3), torch.zeros(8, 25), 8)
    dj, dw = tj.to(DEV), tw.to(DEV)
    for bad in (lambda: build_clips(dj, dw, 1), lambda: build_clips(dj, dw, 801), lambda: build_clips(dj[:, :21], dw, 16),
                lambda: build_clips(dj, dw[:, :78], 16), lambda: build_clips(dj, dw.float(), 16),
                lambda: build_clips(dj, dw[:39], 16), lambda: build_clips(dj, dw, 16, up_axis='x'),
                lambda: build_clips(dj, dw, 16, starts=[30]), lambda: build_clips(dj, dw, 16, starts=[-1]),
                lambda: build_clips(dj, dw, 16, overlap_len=16), lambda: build_clips(dj, dw, 16, stats=(np.zeros(10), np.ones(10))),
                lambda: undistort_keypoints(torch.zeros(4, 2, device=DEV), PROX_K, PROX_DIST),
                lambda: undistort_keypoints(torch.zeros(4, 3, device=DEV), PROX_K[:2], PROX_DIST),
                lambda: visibility_masks(torch.zeros(8, 22, 3, device=DEV), torch.zeros(8, 21, device=DEV), 8),
                lambda: visibility_masks(torch.zeros(8, 22, 3, device=DEV), torch.zeros(7, 25, device=DEV), 8)):
        with pytest.raises(ValueError):
            bad()
