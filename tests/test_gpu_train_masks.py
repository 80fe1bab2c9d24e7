"""GPU: rohm_train_cond / rohm_train_traj_window (csrc/train_masks.hip) against the numpy restatement of the loops' mask rules
(tests/train_masks_ref.py), bit for bit; the refused arguments; the reference's recorded steps (tests/golden/train_loop.npz)
through PoseMaskSchedule on the device."""
import itertools
import random

import numpy as np
import pytest
import torch

from helpers import golden
import train_masks_ref as MR
from rohm_amd import _lib
from rohm_amd.train import masks as M
from test_train_masks_ref import BRANCHES, CASES, bank, recorded_cond, seed_all

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N_VIS, VIS_ROWS_EXTRA = 5, 1


def make(B, T, seed):
    rng = np.random.RandomState(seed)
    src = rng.standard_normal((B, T, 294)).astype(np.float32)
    clean = rng.standard_normal((B, T, 294)).astype(np.float32)
    joint_bits = np.asarray([MR.bits_of(rng.choice(np.arange(1, 22), size=rng.randint(1, 7))) for _ in range(B)], np.uint32)
    start = rng.randint(0, T, size=B)
    window = np.stack([start, np.minimum(start + rng.randint(0, 31, size=B), T)], axis=1).astype(np.int32)
    vis_bits = rng.randint(0, 1 << 22, size=(N_VIS, T + VIS_ROWS_EXTRA)).astype(np.uint32)
    vis_bits[0] = (1 << 22) - 1                      # a clip that hides nothing
    vis_index = rng.randint(0, N_VIS, size=B).astype(np.int64)
    return src, clean, joint_bits, window, vis_bits, vis_index


def run(src, clean=None, **kw):
    cond, clean_t = M.train_cond(torch.from_numpy(src).to(DEV), None if clean is None else torch.from_numpy(clean).to(DEV), **kw)
    return cond.cpu().numpy(), (None if clean_t is None else clean_t.cpu().numpy())


@pytest.mark.parametrize('B,T', list(itertools.product((1, 3), (1, 15, 33, 144))))
def test_every_combination_of_inputs(B, T):
    src, clean, joint_bits, window, vis_bits, vis_index = make(B, T, 100 * B + T)
    for with_j, with_w, with_v, zc, with_clean in itertools.product((False, True), repeat=5):
        kw = dict(zero_contact=zc)
        if with_j:
            kw['joint_bits'] = joint_bits
        if with_w:
            kw['window'] = window
        if with_v:
            kw.update(vis_bits=vis_bits, vis_index=vis_index)
        cond, clean_t = run(src, clean if with_clean else None, **kw)
        assert cond.shape == (B, 294, 1, T)
        assert np.array_equal(cond, MR.train_cond(src, **kw)), (with_j, with_w, with_v, zc, with_clean)
        if with_clean:
            assert np.array_equal(clean_t.view(np.uint32), MR.transpose(clean).view(np.uint32))      # bit for bit
        else:
            assert clean_t is None
    # nothing asked for: the transpose alone, bit for bit
    assert np.array_equal(run(src)[0].view(np.uint32), MR.transpose(src).view(np.uint32))


@pytest.mark.parametrize('T', [15, 144])
def test_windows_joint_sets_and_repeated_clips(T):
    B = 3
    src, clean, _, _, vis_bits, _ = make(B, T, 7)
    for win in ([0, 0], [0, T], [T - 1, T]):
        window = np.asarray([win] * B, np.int32)
        cond, _ = run(src, window=window)
        assert np.array_equal(cond, MR.train_cond(src, window=window))
        n = win[1] - win[0]
        assert int((cond[:, 22:, 0, :] == 0).all(axis=1).sum()) == B * n and np.array_equal(cond[:, :22], MR.transpose(src)[:, :22])
    for joints in ([1], [21], [7], [11], list(range(1, 22))):
        bits = np.full(B, MR.bits_of(joints), np.uint32)
        cond, _ = run(src, joint_bits=bits)
        assert np.array_equal(cond, MR.train_cond(src, joint_bits=bits)), joints
        left, right = cond[:, 290:292].any(), cond[:, 292:].any()
        assert left == (7 not in joints and 10 not in joints) and right == (8 not in joints and 11 not in joints)
        assert cond[:, 280:290].all() and cond[:, :22].all()
    for index in ([2, 2, 2], [4, 0, 4]):
        vi = np.asarray(index, np.int64)
        cond, _ = run(src, vis_bits=vis_bits, vis_index=vi)
        assert np.array_equal(cond, MR.train_cond(src, vis_bits=vis_bits, vis_index=vi)), index
    # the PROX branch multiplies: a hidden negative value becomes -0.0, an infinite one NaN, as `cond * prox_mask` gives
    odd = src.copy()
    odd[0, 0, 22] = -1.0
    odd[0, 0, 25] = np.inf
    vb = vis_bits.copy()
    vb[1, 0] = 0
    cond, _ = run(odd, vis_bits=vb, vis_index=np.asarray([1, 1, 1], np.int64))
    assert np.signbit(cond[0, 22, 0, 0]) and cond[0, 22, 0, 0] == 0 and np.isnan(cond[0, 25, 0, 0])
    cond, _ = run(odd, joint_bits=np.full(B, 0b110, np.uint32))
    assert not np.signbit(cond[0, 22 + 3, 0, 0]) and cond[0, 25, 0, 0] == 0      # an assignment stores +0


@pytest.mark.parametrize('B,T,C,n_ch', [(1, 1, 22, 22), (3, 15, 22, 13), (3, 144, 13, 13), (2, 33, 22, 0)])
def test_traj_window(B, T, C, n_ch):
    rng = np.random.RandomState(T)
    cond = rng.standard_normal((B, T, C)).astype(np.float32)
    for win in ([0, 0], [0, T], [T - 1, T], None):
        if win is None:
            s = rng.randint(0, T, size=B)
            window = np.stack([s, np.minimum(s + rng.randint(0, T + 1, size=B), T)], axis=1).astype(np.int32)
        else:
            window = np.asarray([win] * B, np.int32)
        d = torch.from_numpy(cond).to(DEV)
        out = M.traj_window(d, window, n_ch)
        assert out is d
        assert np.array_equal(d.cpu().numpy(), MR.traj_window(cond, window, n_ch)), win


def test_refused_arguments_raise_before_any_launch():
    B, T = 2, 15
    src, clean, joint_bits, window, vis_bits, vis_index = make(B, T, 3)
    d = torch.from_numpy(src).to(DEV)
    with pytest.raises(_lib.RohmHipError, match=r'vis_index\[1\]=5 outside \[0, 5\)'):
        M.train_cond(d, vis_bits=vis_bits, vis_index=np.asarray([0, 5], np.int64))
    with pytest.raises(_lib.RohmHipError, match=r'vis_index\[0\]=-1 outside'):
        M.train_cond(d, vis_bits=vis_bits, vis_index=np.asarray([-1, 0], np.int64))
    with pytest.raises(_lib.RohmHipError, match='vis_rows=14 is less than T=15'):
        M.train_cond(d, vis_bits=vis_bits[:, :14], vis_index=vis_index)
    with pytest.raises(_lib.RohmHipError, match='T=513 outside'):
        M.train_cond(torch.zeros(1, 513, 294, device=DEV))
    L = _lib.lib()
    out = torch.empty(B, 294, 1, T, device=DEV)
    assert L.rohm_train_cond(_lib.ptr(d), None, -1, T, None, None, None, 0, 0, None, None, 0, _lib.ptr(out), None, None) == -1
    assert b'negative batch size' in L.rohm_last_error()
    assert L.rohm_train_cond(_lib.ptr(d), _lib.ptr(d), B, T, None, None, None, 0, 0, None, None, 0, _lib.ptr(out), None, None) == -1
    assert L.rohm_train_traj_window(_lib.ptr(d), B, T, 294, 295, None, None) == -1
    assert L.rohm_train_traj_window(_lib.ptr(d), -1, T, 294, 4, None, None) == -1
    with pytest.raises(_lib.RohmHipError, match='CPU tensor'):
        M.train_cond(torch.from_numpy(src))
    with pytest.raises(ValueError, match='go together'):
        M.train_cond(d, vis_bits=vis_bits)
    with pytest.raises(ValueError, match='window must have shape'):
        M.train_cond(d, window=np.zeros((3, 2), np.int32))
    # T = 512, the largest supported clip, and an empty batch
    big = np.random.RandomState(0).standard_normal((1, 512, 294)).astype(np.float32)
    w = np.asarray([[500, 512]], np.int32)
    assert np.array_equal(run(big, window=w)[0], MR.train_cond(big, window=w))
    assert M.train_cond(torch.zeros(0, 15, 294, device=DEV))[0].shape == (0, 294, 1, 15)


@pytest.mark.parametrize('name', list(CASES))
def test_recorded_steps_through_the_schedule(name):
    gd = golden('train_loop.npz')
    case, bs = CASES[name], int(gd['bs'])
    b = bank(gd)
    b.device = torch.device(DEV)
    sched = M.PoseMaskSchedule(case['start_prox'], case['scheme'], case['input_noise'], b)
    seed_all(int(gd[f'{name}_seed']))
    log_interval, n_eval = int(gd[f'{name}_log_interval']), 0
    dev = {k: torch.from_numpy(gd[k]).to(DEV) for k in gd.files if k.startswith(('train', 'test0'))}
    for step in range(int(gd[f'{name}_n_steps'])):
        batch = {k: dev[f'train{step % 2}_{k}'] for k in ('motion_repr_clean', 'motion_repr_noisy')}
        d = sched(batch, step // 2)
        np.random.choice(1000, size=(bs,), p=np.ones([1000]) / 1000)      # the loop's timestep draw keeps the generators in step
        assert d.branch == BRANCHES[int(gd[f'{name}_branch'][step])]
        assert np.array_equal(batch['cond'].cpu().numpy(), recorded_cond(gd, name, step)[1]), (name, step)
        assert np.array_equal(batch['motion_repr_clean'].cpu().numpy(), MR.transpose(gd[f'train{step % 2}_motion_repr_clean']))
        if step % log_interval == 0 and step > 0:
            tb = {k: dev[f'test0_{k}'] for k in ('motion_repr_clean', 'motion_repr_noisy')}
            sched(tb, step // 2, eval_block=True)
            assert np.array_equal(tb['cond'].cpu().numpy(), recorded_cond(gd, name, n_eval, 'eval_', 'test0')[1])
            n_eval += 1


def test_recorded_trajnet_steps_through_the_schedule():
    gd = golden('train_loop.npz')
    bs = int(gd['bs'])
    sched = M.TrajMaskSchedule(0, 0.6, 0.5)
    seed_all(int(gd['traj_seed']))
    for step in range(len(gd['traj_cond'])):
        batch = {'cond': torch.from_numpy(gd[f'train{step % 2}_motion_repr_noisy'])[:, :, :22].to(DEV)}
        sched(batch, step // 2, 13)
        np.random.choice(100, size=(bs,), p=np.ones([100]) / 100)
        assert np.array_equal(batch['cond'].cpu().numpy(), gd['traj_cond'][step]), step
