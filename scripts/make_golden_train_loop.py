"""Golden vectors of the training loops -> tests/golden/train_loop.npz and tests/golden/train_cfg/*.yaml.

The reference's own `TrainLoopPoseNet.run_loop` / `TrainLoopTrajNet.run_loop` (train/training_loop_*.py), imported through
oracle.refload with `blobfile` stubbed, run on: a stub model with one parameter; a stub `diffusion_train` whose
`training_losses` records batch['cond'], batch['motion_repr_clean'] and t and returns a differentiable scalar; a stub
`diffusion_eval` that records the eval block's cond; list-like loaders (no DataLoader, so no hidden draws) of random normal
batches, bs = 3, clip_len 16 -> T = 15, 294 channels; a temporary tree with one PROX recording.  `random`, `torch` and
`numpy.random` are seeded at the start of a case.  Cases:
  p1n   phase 1 (random joints), input_noise True, with an eval block every 3 steps
  p1c   phase 1, input_noise False
  p2a   phase 2, mask_scheme 'lower+upper+full', start_prox_mask_epoch -1, input_noise True
  p2l   phase 2, mask_scheme 'lower', start_prox_mask_epoch -1, input_noise True
  traj  TrajNet, start_infill_epoch 0, mask_prob 0.6, max_infill_ratio 0.5 (cond of 22 channels, traj_feat_dim 13)
A recorded PoseNet cond differs from the transposed source rows only where it is 0, so it is stored as the packed bits of
`cond != source` (asserted here to rebuild the recorded array exactly, with np.array_equal); the TrajNet cond is stored whole.
The decisions (branch, joint sets, windows, PROX clips) are read off the recorded arrays here and stored next to them.  The seed
of a case is the first of 0, 1, ... whose steps cover what the case must cover (see `covers`).  The six
cfg_files/train_cfg/*.yaml hold only settings and are copied.  None of the reference's text is here.
Needs a RoHM checkout at oracle.refload.REF_ROOT; run once where it exists, commit only the fixtures:
    python scripts/make_golden_train_loop.py
"""
import importlib
import os
import random
import shutil
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle import refload  # noqa: E402
import train_masks_ref as MR  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
BS, CLIP_LEN, T, C = 3, 16, 15, 294
DATA_SEED, PROX_SEED = 4242, 77
LR = 1e-3


def make_batches(seed, n):
    g = torch.Generator().manual_seed(seed)
    return [{'motion_repr_clean': torch.randn(BS, T, C, generator=g), 'motion_repr_noisy': torch.randn(BS, T, C, generator=g)}
            for _ in range(n)]


def prox_mask(seed):
    """One recording [12 * 16 + 5, 25]: ten clips with about a fifth of the joints hidden, two clips (2 and 7) with too few hidden
    joints to be kept (ratio 0 and 4 / 352), five frames left over."""
    rng = np.random.RandomState(seed)
    m = (rng.rand(12 * CLIP_LEN + 5, 25) > 0.2).astype(np.float64)
    m[2 * CLIP_LEN:3 * CLIP_LEN] = 1.0
    m[7 * CLIP_LEN:8 * CLIP_LEN] = 1.0
    m[7 * CLIP_LEN + 3, [7, 8, 10, 11]] = 0.0
    return m


class Dataset:
    def __init__(self, traj_feat_dim):
        self.clip_len, self.traj_feat_dim = CLIP_LEN, traj_feat_dim


class ListLoader:
    """len() and iteration over fresh dicts of fresh tensors (the loops write into the batch they are given)."""

    def __init__(self, batches, traj_feat_dim=22):
        self.batches, self.dataset = batches, Dataset(traj_feat_dim)

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        for b in self.batches:
            yield {k: v.clone() for k, v in b.items()}


class Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(()))


class Recorder:
    num_timesteps = 1000

    def __init__(self, traj):
        self.traj, self.steps, self.evals = traj, [], []

    def training_losses(self, model, batch, t, noise=None, smplx_model=None, traj_feat_dim=None):
        self.steps.append({'cond': batch['cond'].detach().clone().numpy(), 't': t.clone().numpy(),
                           'clean': batch['motion_repr_clean'].detach().clone().numpy()})
        losses = {'loss': model.w * batch['cond'].abs().mean()}
        return losses if self.traj else (losses, None)

    def eval_losses(self, model, batch, shape, **kw):
        self.evals.append({'cond': batch['cond'].detach().clone().numpy(), 'shape': list(shape)})
        return {'loss': torch.tensor(float(len(self.evals)))}, None


class Quiet:
    def __init__(self):
        self.lines, self.scalars = [], []

    def info(self, msg):
        self.lines.append(msg)

    def add_scalar(self, tag, value, step):
        self.scalars.append((tag, value, step))


def seed_all(seed):
    random.seed(seed)
    torch.manual_seed(seed)
    np.random.seed(seed)


def args_for(tmp, num_steps, log_interval):
    return types.SimpleNamespace(batch_size=BS, lr=LR, log_interval=log_interval, save_interval=10 ** 9, weight_decay=0.0,
                                 body_model_path='unused', num_steps=num_steps, dataset_root=os.path.join(tmp, 'AMASS'))


def run_posenet(loops, tmp, seed, input_noise, start_prox, scheme, train, test, num_steps, log_interval):
    rec, quiet, raw = Recorder(False), Quiet(), []
    real_rand = torch.rand

    def spy(*a, **k):
        out = real_rand(*a, **k)
        raw.append(out.clone().numpy())
        return out
    seed_all(seed)
    torch.rand = spy
    try:
        loops.posenet.TrainLoopPoseNet(args_for(tmp, num_steps, log_interval), writer=quiet, model=Model(), diffusion_train=rec,
                                       diffusion_eval=rec, timestep_respacing_eval='', input_noise=input_noise,
                                       train_dataloader=ListLoader(train), test_dataloader=ListLoader(test), logdir=tmp,
                                       logger=quiet, start_prox_mask_epoch=start_prox, mask_scheme=scheme).run_loop()
    finally:
        torch.rand = real_rand
    return rec, quiet, raw


def hidden_joint_bits(zero):
    """zero [T, 294] bool of one item -> bits of the joints whose position channels are 0 in every frame."""
    return MR.bits_of(j for j in range(22) if zero[:, MR.POS0 + 3 * j:MR.POS0 + 3 * j + 3].all())


def classify(cond, src, bank_bits, phase2, input_noise):
    """Read the decision of one recorded step off its arrays -> dict(branch, joint_bits, window, vis_index, zero_contact)."""
    zero = (cond != MR.transpose(src))[:, :, 0, :].transpose(0, 2, 1)                       # [B, T, 294]
    out = {'branch': 'joints', 'joint_bits': np.zeros(BS, np.uint32), 'window': np.zeros((BS, 2), np.int32),
           'vis_index': np.full(BS, -1, np.int64), 'zero_contact': bool(zero[:, :, MR.CONTACT0:].all())}
    per_frame = [np.unique(z[:, :MR.CONTACT0], axis=0).shape[0] > 1 for z in zero]
    if phase2 and zero[:, :, MR.BETAS0:MR.CONTACT0].any():
        out['branch'] = 'full'
        for b in range(BS):
            f = np.nonzero(zero[b, :, MR.BETAS0])[0]
            assert len(f) and (np.diff(f) == 1).all()
            out['window'][b] = (f[0], f[-1] + 1)
    elif phase2 and any(per_frame):
        out['branch'] = 'prox'
        for b in range(BS):
            hits = [k for k in range(len(bank_bits))
                    if np.array_equal(MR.vis_vector(bank_bits[k][:T])[:, :MR.CONTACT0] == 0, zero[b][:, :MR.CONTACT0])]
            assert len(hits) == 1, hits
            out['vis_index'][b] = hits[0]
    else:
        out['joint_bits'][:] = [hidden_joint_bits(z) for z in zero]
        if phase2:
            assert len(set(out['joint_bits'].tolist())) == 1
            out['branch'] = 'lower' if int(out['joint_bits'][0]) == MR.bits_of(MR.LOWER) else 'upper'
    kw = {}
    if out['branch'] in ('joints', 'lower', 'upper'):
        kw['joint_bits'] = out['joint_bits']
    if out['branch'] == 'full':
        kw['window'] = out['window']
    if out['branch'] == 'prox':
        kw.update(vis_bits=bank_bits, vis_index=out['vis_index'])
    assert np.array_equal(MR.train_cond(src, zero_contact=out['zero_contact'], **kw), cond), 'the decision read off does not rebuild cond'
    return out, zero


BRANCH_ID = {'joints': 0, 'prox': 1, 'lower': 2, 'upper': 3, 'full': 4, 'none': 5}


def store_posenet(out, name, rec, train, test, bank_bits, phase2, input_noise, log_interval):
    key = 'motion_repr_noisy' if input_noise else 'motion_repr_clean'
    n = len(rec.steps)
    dec, zeros = [], []
    for i, st in enumerate(rec.steps):
        b = train[i % len(train)]
        assert np.array_equal(st['clean'], MR.transpose(b['motion_repr_clean'].numpy()))
        d, zero = classify(st['cond'], b[key].numpy(), bank_bits, phase2, input_noise)
        rebuilt = np.where(zero.transpose(0, 2, 1)[:, :, None, :], np.float32(0), MR.transpose(b[key].numpy()))
        assert np.array_equal(rebuilt, st['cond'])
        dec.append(d)
        zeros.append(np.packbits(zero.reshape(-1)))
    out[f'{name}_n_steps'] = np.int64(n)
    out[f'{name}_t'] = np.stack([st['t'] for st in rec.steps])
    out[f'{name}_zero_bits'] = np.stack(zeros)
    out[f'{name}_branch'] = np.asarray([BRANCH_ID[d['branch']] for d in dec], np.int64)
    out[f'{name}_joint_bits'] = np.stack([d['joint_bits'] for d in dec])
    out[f'{name}_window'] = np.stack([d['window'] for d in dec])
    out[f'{name}_vis_index'] = np.stack([d['vis_index'] for d in dec])
    out[f'{name}_zero_contact'] = np.asarray([d['zero_contact'] for d in dec])
    ev_dec, ev_zero = [], []
    for i, ev in enumerate(rec.evals):
        d, zero = classify(ev['cond'], test[i % len(test)][key].numpy(), bank_bits, False, input_noise)
        assert ev['shape'] == [BS, C, 1, T]
        ev_dec.append(d)
        ev_zero.append(np.packbits(zero.reshape(-1)))
    if ev_dec:
        out[f'{name}_eval_zero_bits'] = np.stack(ev_zero)
        out[f'{name}_eval_joint_bits'] = np.stack([d['joint_bits'] for d in ev_dec])
    out[f'{name}_log_interval'] = np.int64(log_interval)
    return dec


def covers(name, dec, raw):
    """What the recorded steps of a case must contain (a condition on the seed, not a measurement)."""
    if name.startswith('p1'):
        drawn = [(r * 22).astype(np.int64) for r in raw]
        bits = np.concatenate([d['joint_bits'] for d in dec])
        left, right = MR.bits_of((7, 10)), MR.bits_of((8, 11))
        return any((d == 0).any() for d in drawn) and (bits & left).any() and (bits & right).any() and \
            len({r.shape[1] for r in raw}) >= 3
    if name == 'p2a':
        ups = [MR.joints_of(d['joint_bits'][0]) for d in dec if d['branch'] == 'upper']
        return {d['branch'] for d in dec} >= {'prox', 'lower', 'upper', 'full'} and \
            any(21 in u and len(u) <= 9 for u in ups) and any(u == sorted(MR.UPPER) for u in ups) and \
            any(d['window'][:, 1].max() == T and (d['window'][:, 1] - d['window'][:, 0]).min() < 30
                for d in dec if d['branch'] == 'full') and sum(d['branch'] == 'prox' for d in dec) >= 3
    if name == 'p2l':
        return {d['branch'] for d in dec} == {'prox', 'lower'} and sum(d['branch'] == 'prox' for d in dec) >= 2
    raise KeyError(name)


def main():
    if not refload.available():
        raise SystemExit(f'needs the reference checkout at {refload.REF_ROOT}')
    sys.modules.setdefault('blobfile', types.ModuleType('blobfile'))
    refload.load()
    loops = types.SimpleNamespace(posenet=importlib.import_module('train.training_loop_posenet'),
                                  trajnet=importlib.import_module('train.training_loop_trajnet'))
    train, test = make_batches(DATA_SEED, 2), make_batches(DATA_SEED + 1, 1)
    mask = prox_mask(PROX_SEED)
    out = {'bs': np.int64(BS), 'clip_len': np.int64(CLIP_LEN), 'prox_mask': mask.astype(np.uint8), 'lr': np.float64(LR)}
    for i, b in enumerate(train):
        for k, v in b.items():
            out[f'train{i}_{k}'] = v.numpy()
    for k, v in test[0].items():
        out[f'test0_{k}'] = v.numpy()
    # the kept clips, by the reference's own rule restated in train_masks_ref
    kept = [i for i in range(len(mask) // CLIP_LEN)
            if (1 - mask[i * CLIP_LEN:(i + 1) * CLIP_LEN, :22].mean()) >= 0.05]
    bank_bits = np.stack([MR.pack_visibility(mask[i * CLIP_LEN:(i + 1) * CLIP_LEN]) for i in kept])
    assert len(kept) == 10 and len({b.tobytes() for b in bank_bits[:, :T]}) == len(kept)
    out['prox_kept'] = np.asarray(kept, np.int64)

    cases = {'p1n': dict(input_noise=True, start_prox=10 ** 6, scheme='lower', num_steps=7, log_interval=3),
             'p1c': dict(input_noise=False, start_prox=10 ** 6, scheme='lower', num_steps=5, log_interval=10 ** 9),
             'p2a': dict(input_noise=True, start_prox=-1, scheme='lower+upper+full', num_steps=27, log_interval=10 ** 9),
             'p2l': dict(input_noise=True, start_prox=-1, scheme='lower', num_steps=7, log_interval=10 ** 9)}
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, 'PROX', 'mask_joint', 'MPH11_00034_01'))
        np.save(os.path.join(tmp, 'PROX', 'mask_joint', 'MPH11_00034_01', 'mask_joint.npy'), mask)
        for name, kw in cases.items():
            for seed in range(200):
                rec, quiet, raw = run_posenet(loops, tmp, seed, kw['input_noise'], kw['start_prox'], kw['scheme'], train, test,
                                              kw['num_steps'], kw['log_interval'])
                scratch = {}
                dec = store_posenet(scratch, name, rec, train, test, bank_bits, kw['start_prox'] < 0, kw['input_noise'],
                                    kw['log_interval'])
                if covers(name, dec, raw):
                    break
            else:
                raise SystemExit(f'no seed below 200 covers case {name}')
            out.update(scratch)
            out[f'{name}_seed'] = np.int64(seed)
            out[f'{name}_num_steps'] = np.int64(kw['num_steps'])
            out[f'{name}_log_lines'] = np.asarray(quiet.lines)
            print(name, 'seed', seed, 'steps', len(rec.steps), 'evals', len(rec.evals), 'branches',
                  [d['branch'] for d in dec])

        # ---- TrajNet
        traj_train = [dict(b, cond=b['motion_repr_noisy'][:, :, :22].clone()) for b in train]
        for seed in range(200):
            rec, quiet = Recorder(True), Quiet()
            rec.num_timesteps = 100
            seed_all(seed)
            loops.trajnet.TrainLoopTrajNet(args_for(tmp, 9, 10 ** 9), writer=quiet, model=Model(), diffusion_train=rec,
                                           diffusion_eval=rec, timestep_respacing_eval='', start_infill_epoch=0,
                                           max_infill_ratio=0.5, mask_prob=0.6, train_dataloader=ListLoader(traj_train, 13),
                                           test_dataloader=ListLoader(test, 13), logdir=tmp, logger=quiet).run_loop()
            conds = np.stack([st['cond'] for st in rec.steps])
            windows, masked = [], []
            for i, st in enumerate(rec.steps):
                src = traj_train[i % 2]['cond'].numpy()
                zero = (st['cond'] != src)
                assert not zero[:, :, 13:].any()
                w = np.zeros((BS, 2), np.int32)
                for b in range(BS):
                    f = np.nonzero(zero[b, :, 0])[0]
                    if len(f):
                        assert (np.diff(f) == 1).all()
                        w[b] = (f[0], f[-1] + 1)
                assert np.array_equal(MR.traj_window(src, w, 13), st['cond'])
                windows.append(w)
                masked.append(bool(zero.any()))
            lens = np.concatenate([w[:, 1] - w[:, 0] for w in windows])
            if sum(masked) >= 3 and not all(masked) and (lens == 0).any() and lens.max() >= 5 and \
                    any((w[:, 1] == T).any() for w in windows):
                break
        else:
            raise SystemExit('no seed below 200 covers the TrajNet case')
        out.update(traj_seed=np.int64(seed), traj_num_steps=np.int64(9), traj_cond=conds, traj_window=np.stack(windows),
                   traj_masked=np.asarray(masked), traj_t=np.stack([st['t'] for st in rec.steps]))
        print('traj seed', seed, 'masked', masked)

    path = os.path.join(GOLD, 'train_loop.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))
    assert os.path.getsize(path) < 1000000, 'fixtures stay under 1 MB'
    cfg_src, cfg_dst = os.path.join(refload.REF_ROOT, 'cfg_files', 'train_cfg'), os.path.join(GOLD, 'train_cfg')
    os.makedirs(cfg_dst, exist_ok=True)
    for f in sorted(os.listdir(cfg_src)):
        if f.endswith('.yaml'):
            shutil.copyfile(os.path.join(cfg_src, f), os.path.join(cfg_dst, f))
            print('copied', f)


if __name__ == '__main__':
    main()
