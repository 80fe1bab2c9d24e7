"""Golden vectors of the AMASS loader -> tests/golden/amass_loader.npz.

The reference's own `DataloaderAMASS` (data_loaders/dataloader_amass.py) on the synthetic tree of tests/amass_ref.py (two
datasets, sequences of 40, 12 and 33 frames, clip_len 16 -> 4 train clips, 3 test clips): the tree's arrays, the noise, the
pickled statistics, every intermediate list and every item of four cases:
  a  split 'train', task 'pose', noise drawn after np.random.seed(SEED_A) at the stage-1 stds (1, 1, 0.01, 0.01);
  b  split 'test', spacing 2, load_noise with a noise dict drawn after np.random.seed(SEED_B) at the stage-2 stds
     (2, 2, 0.03, 0.2), task 'traj' with repr_abs_only;
  c  split 'train', input_noise=False, task 'traj';
  d  split 'train', sep_noise (noise_std_joint 1e-4, small parameter stds), task 'traj', items after np.random.seed(SEED_D).
The body model is the oracle's (registered with `refload.set_body_model`) behind a wrapper that flattens `body_pose`
[T,21,3], which the reference passes as it is.  The reference is imported through oracle.refload; none of its text is here.
Needs a RoHM checkout at oracle.refload.REF_ROOT; run once where it exists, commit only the .npz file:
    python scripts/make_golden_amass.py            (`scan` as argument: print the margins of seeds 0..11 and stop)
"""
import importlib
import os
import pickle
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle import geometry as G  # noqa: E402
from oracle import refload  # noqa: E402
from rohm_amd.utils import synth  # noqa: E402
import amass_ref as AR  # noqa: E402
import clips_ref as CR  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
SEED_A, SEED_B, SEED_D = AR.SEED_A, AR.SEED_B, AR.SEED_D
DATASETS = list(AR.TREE)


class FlatBodyPose(torch.nn.Module):
    def __init__(self, body):
        super().__init__()
        self.body = body

    def forward(self, **kw):
        kw['body_pose'] = kw['body_pose'].reshape(kw['body_pose'].shape[0], -1)
        return self.body(**kw)


def loader(da, root, logdir, **kw):
    return da.DataloaderAMASS(preprocessed_amass_root=root, body_model_path='unused', amass_datasets=DATASETS,
                              clip_len=AR.CLIP_LEN, logdir=logdir, device='cpu', **kw)


def stage2_noise_dict(seed, rows=5):
    """What the reference pickles as its noise file ([rows, L, ...] per parameter), drawn like its own loop draws."""
    np.random.seed(seed)
    per = [AR.draw_noise(AR.CLIP_LEN, AR.std_dict(AR.STAGE2_STD)) for _ in range(rows)]
    return {k: np.asarray([p[k] for p in per]) for k in AR.NOISE_ORDER}


def lists(ds, noisy):
    out = {'joints_clean': np.asarray(ds.joints_clean_list), 'repr_clean': np.concatenate([ds.repr_list_dict[k] for k in G.REPR_LIST], -1)}
    for k in AR.PARAM_NAMES:
        out['params_' + k] = np.asarray(ds.smplx_params_list_dict[k])
    if noisy:
        out['joints_noisy'] = np.asarray(ds.joints_noisy_list)
        out['repr_noisy'] = np.concatenate([np.asarray(ds.repr_list_dict_noisy[k]) for k in G.REPR_LIST], -1)
    return out


def noisy_side(ds, noise):
    """The noisy parameters are not kept by the reference: recompute them with its own scipy calls from its canonical
    parameters and the recorded noise, and check them through the joints it did keep."""
    n = len(ds.joints_clean_list)
    params = [{k: ds.smplx_params_list_dict[k][i] for k in AR.PARAM_NAMES} for i in range(n)]
    noisy = [AR.perturb_params(p, {k: noise[k][i] for k in AR.NOISE_ORDER}) for i, p in enumerate(params)]
    from oracle import frames as OF
    for i, q in enumerate(noisy):
        fk = OF.noisy_clip_joints(refload._body_model.body, {k: np.asarray(v).reshape(AR.CLIP_LEN, -1) for k, v in q.items()})
        assert np.array_equal(fk, ds.joints_noisy_list[i]), 'noisy parameters do not reproduce the recorded noisy joints'
    return params, noisy


def check_case(name, clean_joints, noisy_joints, params, noisy_params, clean_repr, noisy_repr, want_noisy_contact):
    assert not np.isnan(clean_repr).any() and set(np.unique(clean_repr[..., 290:])) == {0.0, 1.0}, name
    msg = [name]
    if noisy_repr is not None:
        assert not np.isnan(noisy_repr).any(), name
        near = AR.near_threshold(noisy_joints)
        msg.append(f'near-threshold decisions {int(near.sum())} of {near.size}')
        assert near.mean() <= 0.01, (name, near.sum(), near.size)
        vals = set(np.unique(noisy_repr[..., 290:]))
        msg.append(f'noisy contact values {sorted(vals)}')
        if want_noisy_contact:
            assert vals == {0.0, 1.0}, name
    if noisy_params is not None:
        mid, ang = AR.euler_margins(params, noisy_params)
        msg.append(f'Euler middle angle {mid:.1f} deg from +-90, rotation angle {ang:.3f} rad from pi')
        assert mid > 5.0 and ang > 1e-3, (name, mid, ang)
    print('; '.join(msg))


def put_items(out, p, ds, n, skip=()):
    """Every item of the loader.  `cond` / `control_cond` are asserted to be the slices of the item's own rows that
    dataloader_amass.py:331-339 takes and are not stored."""
    for i in range(n):
        item = ds[i]
        assert list(item) == [k for k in ('motion_repr_clean', 'noisy_joints', 'motion_repr_noisy', 'cond', 'control_cond')
                              if k in item], list(item)
        assert ('cond' in item) == ('control_cond' in item) == (ds.task == 'traj') and ('noisy_joints' in item) == ds.input_noise
        if ds.task == 'traj':
            t = item['motion_repr_noisy']
            assert np.array_equal(item['cond'], t[:, AR.ABS_TRAJ_CH] if ds.repr_abs_only else t[:, :22])
            assert np.array_equal(item['control_cond'], item['motion_repr_clean'][:, -272:])
            assert item['cond'].dtype == item['control_cond'].dtype == np.float32
        for k, v in item.items():
            if k not in skip and k not in ('cond', 'control_cond'):
                out[f'{p}item{i}_{k}'] = np.asarray(v)


def scan(da, root, tmp):
    for seed in range(12):
        np.random.seed(seed)
        a = loader(da, root, os.path.join(tmp, f'scan{seed}'), split='train', task='pose', input_noise=True, **AR.STAGE1_STD)
        na = AR.near_threshold(np.asarray(a.joints_noisy_list))
        ca = sorted(set(np.unique(np.concatenate([a.repr_list_dict_noisy['foot_contact'][i] for i in range(4)]))))
        b = loader(da, root, os.path.join(tmp, f'scan{seed}'), split='test', spacing=2, task='traj', repr_abs_only=True,
                   input_noise=True, load_noise=True, loaded_smplx_noise_dict=stage2_noise_dict(seed), **AR.STAGE2_STD)
        nb = AR.near_threshold(np.asarray(b.joints_noisy_list))
        print(f'seed {seed}: stage 1 near {int(na.sum())}/{na.size} contact {ca}; stage 2 near {int(nb.sum())}/{nb.size}')


def main():
    if not refload.available():
        raise SystemExit(f'needs the reference checkout at {refload.REF_ROOT}')
    ref = refload.load()
    refload.set_body_model(FlatBodyPose(G.BodyModel(synth.synthetic_smplx_tensors(0))))
    da = importlib.import_module('data_loaders.dataloader_amass')
    arrays = AR.tree_arrays()
    out = {'clip_len': np.int64(AR.CLIP_LEN), 'seed_a': np.int64(SEED_A), 'seed_b': np.int64(SEED_B), 'seed_d': np.int64(SEED_D)}
    for key, (joints, smplx) in arrays.items():
        out['tree_' + key.replace('/', '__') + '_joints'] = joints[:, :22]
        out['tree_' + key.replace('/', '__') + '_smplx'] = smplx[:, :79]
    with tempfile.TemporaryDirectory() as tmp:
        root, logdir = AR.write_tree(os.path.join(tmp, 'amass'), arrays), os.path.join(tmp, 'log')
        if sys.argv[1:] == ['scan']:
            return scan(da, root, tmp)

        # ---- a: train, task 'pose', drawn noise
        np.random.seed(SEED_A)
        a = loader(da, root, logdir, split='train', task='pose', input_noise=True, **AR.STAGE1_STD)
        assert a.n_samples == 4 and len(a) == 4
        np.random.seed(SEED_A)
        noise_a = [AR.draw_noise(AR.CLIP_LEN, AR.std_dict(AR.STAGE1_STD)) for _ in range(4)]
        noise_a = {k: np.asarray([p[k] for p in noise_a]) for k in AR.NOISE_ORDER}
        la = lists(a, True)
        params, noisy = noisy_side(a, noise_a)             # asserts that noise_a is what the loader drew
        check_case('a', la['joints_clean'], la['joints_noisy'], params, noisy, la['repr_clean'], la['repr_noisy'], True)
        for k, v in la.items():
            out['a_' + k] = v
        for k in AR.NOISE_ORDER:
            out['a_noise_' + k] = noise_a[k]
            out['a_noisy_' + k] = np.asarray([q[k] for q in noisy])
        out['a_transf'] = np.asarray([ref.motion_repr.cano_seq_smplx(
            positions=j.copy(), smplx_params_dict={k: v.copy() for k, v in p.items()}, return_transf_mat=True)[2]
            for j, p in AR.read_clips(root, DATASETS, 'train', AR.CLIP_LEN)])
        put_items(out, 'a_', a, 4)
        for attr in ('body_feat_dim', 'traj_feat_dim', 'pose_feat_dim', 'n_samples', 'clip_len'):
            out['a_' + attr] = np.int64(getattr(a, attr))
        # the statistics and their pickles
        for fname, tag in (('AMASS_mean.pkl', 'mean'), ('AMASS_std.pkl', 'std')):
            with open(os.path.join(logdir, fname), 'rb') as f:
                out[tag + '_pkl'] = np.frombuffer(f.read(), dtype=np.uint8)
        out['Mean'], out['Std'] = a.Mean, a.Std
        flat = la['repr_clean'].reshape(-1, 294).astype(np.float64)
        m64, s64 = flat.mean(axis=0), flat.std(axis=0)
        s64g = s64.copy()
        for name, (lo, hi) in AR.GROUPS.items():
            if name == 'foot_contact':
                m64[lo:hi], s64g[lo:hi] = 0.0, 1.0
            elif name != 'smplx_betas':
                s64g[lo:hi] = s64[lo:hi].mean()
        dm, dstd = np.abs(a.Mean - m64).max(), np.abs(a.Std - s64g).max()
        print(f'statistics: float32-accumulated vs float64: Mean {dm:.3e}, Std {dstd:.3e}; smallest Std {a.Std.min():.3e}')
        out['mean_bar'], out['std_bar'] = np.float64(4 * dm), np.float64(4 * dstd)

        # ---- b: test, spacing 2, loaded noise, task 'traj' with repr_abs_only
        noise_b = stage2_noise_dict(SEED_B)
        b = loader(da, root, logdir, split='test', spacing=2, task='traj', repr_abs_only=True, input_noise=True, load_noise=True,
                   loaded_smplx_noise_dict=noise_b, **AR.STAGE2_STD)
        assert b.n_samples == 3 and len(b) == 1 and len(b.joints_clean_list) == 2
        lb = lists(b, True)
        used = {k: noise_b[k][[0, 4]] for k in AR.NOISE_ORDER}      # rows i * spacing for i = 0, 2
        params, noisy = noisy_side(b, used)
        check_case('b', lb['joints_clean'], lb['joints_noisy'], params, noisy, lb['repr_clean'], lb['repr_noisy'], False)
        for k, v in lb.items():
            out['b_' + k] = v
        for k in AR.NOISE_ORDER:
            out['b_noise_' + k] = noise_b[k]
            out['b_noisy_' + k] = np.asarray([q[k] for q in noisy])
        put_items(out, 'b_', b, 2)
        for attr in ('traj_feat_dim', 'pose_feat_dim', 'n_samples'):
            out['b_' + attr] = np.int64(getattr(b, attr))
        out['b_len'] = np.int64(len(b))

        # ---- c: no input noise (the clean lists are case a's)
        c = loader(da, root, os.path.join(tmp, 'log_c'), split='train', task='traj', input_noise=False)
        assert np.array_equal(lists(c, False)['repr_clean'], la['repr_clean']) and np.array_equal(c.Mean, a.Mean)
        for i in range(4):                                  # nothing new to store: the items are case a's clean items
            assert np.array_equal(c[i]['motion_repr_noisy'], c[i]['motion_repr_clean'])
            assert np.array_equal(c[i]['motion_repr_clean'], out[f'a_item{i}_motion_repr_clean'])
        put_items(out, 'c_', c, 4, skip=('motion_repr_noisy', 'motion_repr_clean'))

        # ---- d: sep_noise (the clean lists are case a's)
        d = loader(da, root, os.path.join(tmp, 'log_d'), split='train', task='traj', input_noise=True, sep_noise=True,
                   noise_std_joint=AR.SEP_STD_JOINT, **AR.SEP_STD)
        np.random.seed(SEED_D)
        put_items(out, 'd_', d, 4, skip=('motion_repr_clean',))
        rd = np.stack([out[f'd_item{i}_motion_repr_noisy'] for i in range(4)]) * a.Std + a.Mean
        jd = np.stack([out[f'd_item{i}_noisy_joints'] for i in range(4)])
        check_case('d', la['joints_clean'], jd, None, None, la['repr_clean'], rd, True)
    path = os.path.join(GOLD, 'amass_loader.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))
    assert os.path.getsize(path) < 1000000, 'fixtures stay under 1 MB'


if __name__ == '__main__':
    main()
