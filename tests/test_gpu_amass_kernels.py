"""GPU: the kernels behind the native AMASS loader -- rohm_clips_repr, rohm_smplx_param_noise, rohm_repr_stats and
rohm_amass_batch (csrc/clips.hip, csrc/amass.hip) -- against the numpy / scipy restatement (tests/amass_ref.py, pinned to the
reference's loader by tests/test_amass_ref.py) at shapes the loader fixture does not reach."""
import functools

import numpy as np
import pytest
import torch

import amass_ref as AR
import clips_ref as CR
from rohm_amd.utils import synth

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LOCAL_FACTOR = 4 * 0.0112       # tests/test_gpu_clips.py::_close
PARAM_TOL = 1e-9                # float64 Euler round trip of angles up to 180: orders above rounding, below the float32 cast


def _close(out, ref, cano, tol=2e-5):
    """tests/test_gpu_clips.py::_close."""
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    lim = CR.repr_limits(ref, np.asarray(cano, np.float64), None, tol, LOCAL_FACTOR)
    err = np.abs(out - ref)
    assert (err <= lim).all(), f'max err {err.max():.3e}; outside tolerance at {np.argwhere(err > lim)[:5].tolist()}'
    assert np.array_equal(out[..., 290:], ref[..., 290:].astype(np.float32))


@functools.lru_cache(maxsize=None)
def _canonical(N, L, ov):
    """Canonical clips of a synthetic recording: (joints [C,L,22,3] float64, params [C,L,79] float64, list of param dicts)."""
    jw, world = synth.synthetic_recording(21, N, 'z')
    ref = CR.build_clips(jw, world, L, ov, 'z')
    prm = []
    for c, s in enumerate(ref['starts']):
        p = CR.split_world(world[s:s + L])
        p['global_orient'], p['transl'] = ref['global_orient'][c], ref['transl'][c]
        prm.append(p)
    return ref['cano_joints'], np.stack([AR.rows79(p) for p in prm]), prm


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('N,L,ov', [(431, 145, 2), (300, 300, 2), (40, 2, 0)])
def test_clips_repr_vs_restatement(N, L, ov, dtype):
    from rohm_amd._lib import lib
    from rohm_amd.data_loaders.clips import clips_repr
    cano, rows, prm = _canonical(N, L, ov)
    pos = cano.astype(dtype)
    assert len(pos) == {145: 3, 300: 1, 2: 20}[L] and (lib().rohm_clips_scratch_bytes(1, L) > 0) == (L == 300)
    assert CR.contact_margin(pos) > 1e-3
    ref = np.stack([AR.full_repr(p, q) for p, q in zip(pos, prm)])
    assert set(np.unique(ref[..., 290:])) <= {0.0, 1.0} and not np.isnan(ref).any()
    out = clips_repr(torch.from_numpy(pos).to(DEV), torch.from_numpy(rows).to(DEV))
    assert out.shape == (len(pos), L - 1, 294) and out.dtype == torch.float32
    _close(out.cpu().numpy(), ref, pos)
    stats = synth.synthetic_stats(3)
    norm = clips_repr(torch.from_numpy(pos).to(DEV), torch.from_numpy(rows).to(DEV), stats=stats).cpu().numpy()
    _close(norm, (ref - stats[0]) / stats[1], pos)          # as tests/test_gpu_clips.py normalises


def test_clips_repr_joint_noise_and_reproducibility():
    from rohm_amd.data_loaders.clips import clips_repr
    cano, rows, prm = _canonical(431, 145, 2)
    g = np.random.Generator(np.random.PCG64(4))
    noise = g.normal(0.0, 1e-4, size=cano.shape)
    for pos in (cano, cano.astype(np.float32)):
        want = (pos.astype(np.float64) + noise).astype(np.float32)
        out, joints = clips_repr(torch.from_numpy(pos).to(DEV), torch.from_numpy(rows).to(DEV),
                                 joint_noise=torch.from_numpy(noise).to(DEV), return_joints=True)
        assert joints.dtype == torch.float32 and np.array_equal(joints.cpu().numpy(), want)
        ref = np.stack([AR.full_repr(p, q) for p, q in zip(want, prm)])
        near = AR.near_threshold(want)
        err = np.abs(out.cpu().numpy().astype(np.float64) - ref)
        lim = CR.repr_limits(ref, want.astype(np.float64), None, 2e-5, LOCAL_FACTOR)
        assert (err[..., :290] <= lim[..., :290]).all()
        assert np.array_equal(out.cpu().numpy()[..., 290:][~near], ref[..., 290:][~near].astype(np.float32)) and near.mean() <= 0.01
        again = clips_repr(torch.from_numpy(want).to(DEV), torch.from_numpy(rows).to(DEV))
        assert torch.equal(again, out)                      # float32(positions + noise) first, then the float32 flow


def _rotations(M, seed):
    """[M,79] parameter rows whose 22 rotations are spread over the sphere (angles up to pi - 0.05) and noise in degrees such
    that every clean and noisy Euler middle angle stays 5 degrees from +-90 and every noisy angle 1e-3 rad from pi."""
    from scipy.spatial.transform import Rotation as R
    g = np.random.Generator(np.random.PCG64(seed))
    v = g.standard_normal((M * 22, 3))
    v *= g.uniform(0.0, np.pi - 0.05, (M * 22, 1)) / np.linalg.norm(v, axis=1, keepdims=True)
    v[::50] = 0.0                                           # exact identities and small angles (scipy's series branch)
    v[1::50] *= 1e-5
    nz = g.normal(0.0, 2.0, size=v.shape)
    e = R.from_rotvec(v).as_euler('zxy', degrees=True)
    noisy = AR.perturb_rotvec(v, nz)
    bad = (np.abs(e[:, 1]) > 85) | (np.abs(e[:, 1] + nz[:, 1]) > 85) | (np.linalg.norm(noisy, axis=1) > np.pi - 1e-3)
    v[bad] *= 0.3
    e = R.from_rotvec(v).as_euler('zxy', degrees=True)
    noisy = AR.perturb_rotvec(v, nz)
    assert ((np.abs(e[:, 1]) < 85) & (np.abs(e[:, 1] + nz[:, 1]) < 85) & (np.linalg.norm(noisy, axis=1) < np.pi - 1e-3)).all()
    assert np.linalg.norm(v, axis=1).max() > 3.0 and bad.mean() < 0.2
    v, nz = v.reshape(M, 22, 3), nz.reshape(M, 22, 3)
    params = {'global_orient': v[:, 0], 'body_pose': v[:, 1:].reshape(M, 63), 'transl': g.standard_normal((M, 3)),
              'betas': g.standard_normal((M, 10))}
    noise = {'global_orient': nz[:, 0], 'body_pose': nz[:, 1:], 'transl': g.normal(0, 0.03, (M, 3)), 'betas': g.normal(0, 0.2, (M, 10))}
    return params, noise


def test_param_noise_vs_scipy():
    from rohm_amd.data_loaders.dataloader_amass import param_noise
    M = 301                                                 # 6622 rotations: 26 workgroups, the last one partial
    params, noise = _rotations(M, 0)
    ref = AR.rows79(AR.perturb_params(params, noise))
    dev = lambda d: {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in d.items()}
    rows = torch.from_numpy(AR.rows79(params)).to(DEV)
    out = param_noise(rows, dev(noise))
    assert out.dtype == torch.float64 and out.shape == (M, 79)
    assert np.abs(out.cpu().numpy() - ref).max() <= PARAM_TOL
    assert np.linalg.norm(out.cpu().numpy()[:, 16:].reshape(-1, 3), axis=1).max() <= np.pi
    # [C, L, 79] rows and noise for body_pose given as [.., 63]: the same numbers
    n3 = dev(noise)
    n3 = {k: v.reshape((7, 43) + tuple(v.shape[1:])) for k, v in n3.items()}
    n3['body_pose'] = n3['body_pose'].reshape(7, 43, 63)
    assert torch.equal(param_noise(rows.reshape(7, 43, 79), n3).reshape(M, 79), out)
    # zero noise: a round trip through the Euler angles
    zero = {k: torch.zeros_like(v) for k, v in dev(noise).items()}
    assert np.abs(param_noise(rows, zero).cpu().numpy() - AR.rows79(params)).max() <= PARAM_TOL
    # additive: the sep_noise items, plain float64 sums
    flat = dict(noise, body_pose=noise['body_pose'].reshape(M, 63))
    add = param_noise(rows, dev(flat), additive=True).cpu().numpy()
    assert np.array_equal(add, AR.rows79({k: params[k] + flat[k] for k in params}))


@pytest.mark.parametrize('n,L', [(1, 2), (3, 16), (3, 145), (456, 145)])
def test_repr_stats_vs_numpy_and_deterministic(n, L):
    """1 and 45 rows (one workgroup), 432 rows (7 workgroups), 65664 rows (more than 1024 blocks of 64: the blocks grow)."""
    from rohm_amd._lib import lib
    from rohm_amd.data_loaders.dataloader_amass import repr_stats
    rows = n * (L - 1)
    assert lib().rohm_repr_stats_scratch_bytes(rows) == {1: 1, 45: 1, 432: 7, 65664: 513}[rows] * 2 * 294 * 8
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(n, L - 1, 294, generator=g) * torch.linspace(1e-3, 2.0, 294) + torch.linspace(-3.0, 3.0, 294)
    mean, std = repr_stats(x.to(DEV))
    assert mean.dtype == std.dtype == torch.float64 and mean.shape == std.shape == (294,)
    flat = x.double().reshape(-1, 294).numpy()
    # float64 sums of `rows` float32 values of size <= 10: rounding errors of 1e-16 relative per term, far below 1e-12
    assert np.abs(mean.cpu().numpy() - flat.mean(0)).max() <= 1e-12 and np.abs(std.cpu().numpy() - flat.std(0)).max() <= 1e-12
    if rows == 1:
        assert (std == 0).all()
    mean2, std2 = repr_stats(x.to(DEV))
    assert torch.equal(mean, mean2) and torch.equal(std, std2)


def test_assemble_vs_numpy():
    from rohm_amd.data_loaders.dataloader_amass import assemble
    g = torch.Generator().manual_seed(5)
    clean, noisy = torch.randn(5, 15, 294, generator=g), torch.randn(5, 15, 294, generator=g)
    mean, std = (torch.from_numpy(s) for s in synth.synthetic_stats(2))
    idx = torch.tensor([4, 0, 4, 7, -1, 2])
    d = lambda t: t.to(DEV)
    norm = lambda x: ((x.double().numpy() - mean.numpy()) / std.numpy()).astype(np.float32)
    valid = [0, 1, 2, 5]
    src = idx[valid]
    for over, cond in ((0, 'traj'), (22, None), (13, 'abs')):
        out = assemble(d(clean), d(noisy), d(idx), d(mean), d(std), over, cond, control=cond is not None)
        want_noisy = noisy[src].clone()
        want_noisy[..., :over] = clean[src][..., :over]
        c, z = out['motion_repr_clean'].cpu().numpy(), out['motion_repr_noisy'].cpu().numpy()
        assert np.array_equal(c[valid], norm(clean[src])) and np.array_equal(z[valid], norm(want_noisy))
        assert np.isnan(c[[3, 4]]).all() and np.isnan(z[[3, 4]]).all()          # indices outside the dataset
        assert set(out) == {'motion_repr_clean', 'motion_repr_noisy'} | ({'cond', 'control_cond'} if cond else set())
        if cond:
            cols = list(range(22)) if cond == 'traj' else AR.ABS_TRAJ_CH
            assert np.array_equal(out['cond'].cpu().numpy()[valid], z[valid][..., cols])
            assert np.array_equal(out['control_cond'].cpu().numpy()[valid], c[valid][..., -272:])
    # without noisy rows the noisy item is the clean one; per-batch noisy rows are addressed by the batch position
    out = assemble(d(clean), None, d(src), d(mean), d(std))
    assert torch.equal(out['motion_repr_noisy'], out['motion_repr_clean'])
    out = assemble(d(clean), d(noisy[:4]), d(src), d(mean), d(std), noisy_per_batch=True)
    assert np.array_equal(out['motion_repr_noisy'].cpu().numpy(), norm(noisy[:4]))
    assert assemble(d(clean), d(noisy), d(idx[:0]), d(mean), d(std))['motion_repr_clean'].shape == (0, 15, 294)


def test_refused_arguments():
    from rohm_amd._lib import RohmHipError
    from rohm_amd.data_loaders.clips import clips_repr
    from rohm_amd.data_loaders.dataloader_amass import assemble, param_noise, repr_stats
    pos, rows = torch.zeros(2, 16, 22, 3), torch.zeros(2, 16, 79, dtype=torch.float64)
    nz = {'global_orient': torch.zeros(2, 16, 3, dtype=torch.float64), 'transl': torch.zeros(2, 16, 3, dtype=torch.float64),
          'betas': torch.zeros(2, 16, 10, dtype=torch.float64), 'body_pose': torch.zeros(2, 16, 63, dtype=torch.float64)}
    rep, mean = torch.zeros(2, 15, 294), torch.ones(294)
    idx = torch.zeros(2, dtype=torch.int64)
    for cpu_call in (lambda: clips_repr(pos, rows), lambda: param_noise(rows, nz), lambda: repr_stats(rep),
                     lambda: assemble(rep, None, idx, mean, mean)):
        with pytest.raises(RohmHipError):
            cpu_call()
    d = lambda t: t.to(DEV)
    dpos, drows, drep, dmean, didx = d(pos), d(rows), d(rep), d(mean), d(idx)
    dnz = {k: d(v) for k, v in nz.items()}
    bad = [lambda: clips_repr(dpos[:, :, :21], drows), lambda: clips_repr(dpos.half(), drows), lambda: clips_repr(dpos, drows.float()),
           lambda: clips_repr(dpos, drows[:1]), lambda: clips_repr(dpos[:, :1], drows[:, :1]),
           lambda: clips_repr(dpos, drows, joint_noise=dpos), lambda: clips_repr(dpos, drows, stats=(np.zeros(3), np.ones(3))),
           lambda: param_noise(drows.float(), dnz), lambda: param_noise(drows[..., :78], dnz),
           lambda: param_noise(drows, dict(dnz, transl=dnz['transl'].float())),
           lambda: param_noise(drows, dict(dnz, betas=dnz['betas'][:1])),
           lambda: repr_stats(drep.double()), lambda: repr_stats(drep[..., :293]), lambda: repr_stats(drep[:0]),
           lambda: assemble(drep, None, didx.int(), dmean, dmean), lambda: assemble(drep, drep[:1], didx, dmean, dmean),
           lambda: assemble(drep, None, didx, dmean[:10], dmean), lambda: assemble(drep, None, didx, dmean, dmean, cond='both'),
           lambda: assemble(drep, None, didx, dmean, dmean, overwrite_channels=295), lambda: assemble(drep.double(), None, didx, dmean, dmean)]
    for call in bad:
        with pytest.raises(ValueError):
            call()
