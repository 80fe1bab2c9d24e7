"""Time the mask block of a PoseNet training step at B = 64, T = 144 for each branch of the schedule, two ways:

  native   PoseMaskSchedule.apply: the step's decision in one host-to-device copy, then one rohm_train_cond launch that writes the
           masked cond [B, 294, 1, T] and the transposed motion_repr_clean;
  indexed  the same decision applied the way train/training_loop_posenet.py:107-205 writes it: a clone, per-item indexed
           assignments with host index tensors (the PROX branch: np.random.shuffle of a host float64 array [n_clips, 145, 294] in
           place, upload of bs clips, a multiply), then the two permute(0, 2, 1).unsqueeze(-2) made contiguous -- in the reference
           they stay views and the copy happens in the first consumer; here both sides end with the tensors the model reads.

Both sides produce the same bits (checked before timing).  They are warmed up, then alternate in windows of about 0.1 s that end in a device
synchronise until each side has at least --min-seconds.  A whole PoseNet training step (mask block + training_losses + backward +
AdamW) is timed the same way for the mask block's share; the native training path takes T <= 143, so the step runs at
--step-T (143); --optimizer native runs that step with rohm_amd.optim.AdamW instead of torch.optim.AdamW (the default, and what
the loops use unless asked) and adds the two optimisers' whole steps alternating.  Writes profiles/train_loop_timing.json.  Needs the GPU: there is no CPU fallback and no number without a run.

    python scripts/bench_train_loop.py [--B 64] [--T 144] [--min-seconds 1.0] [--prox-clips 500] [--optimizer torch|native]
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rohm_amd.train import masks as M  # noqa: E402
from rohm_amd.utils import synth  # noqa: E402

TRAJ = 22


def indexed_block(d, src, clean, prox_host, input_noise):
    """The reference's mask block for the decision d, restated with its own indexing."""
    cond = src.clone()
    bs = cond.shape[0]
    if d.branch == 'joints':
        ids = torch.tensor(d.joints)                                  # [bs, n] on the host, as mask_joint_id is
        for i in range(bs):
            for k in range(3):
                cond[i, :, TRAJ + ids[i] * 3 + k] = 0.
            for k in range(3):
                cond[i, :, TRAJ + 22 * 3 + ids[i] * 3 + k] = 0.
            for k in range(6):
                cond[i, :, TRAJ + 22 * 3 + 22 * 3 + (ids[i] - 1) * 6 + k] = 0.
            if 7 in ids[i] or 10 in ids[i]:
                cond[i, :, -4:-2] = 0.
            if 8 in ids[i] or 11 in ids[i]:
                cond[i, :, -2:] = 0.
    elif d.branch == 'prox':
        np.random.shuffle(prox_host)
        prox_mask = torch.from_numpy(prox_host[0:bs]).float().to(cond.device)[:, 0:-1]
        cond = cond * prox_mask
    elif d.branch in ('lower', 'upper'):
        ids = np.asarray(d.joints)
        for k in range(3):
            cond[:, :, TRAJ + ids * 3 + k] = 0.
        for k in range(3):
            cond[:, :, TRAJ + 22 * 3 + ids * 3 + k] = 0.
        for k in range(6):
            cond[:, :, TRAJ + 22 * 3 + 22 * 3 + (ids - 1) * 6 + k] = 0.
        cond[:, :, -4:] = 0.
    elif d.branch == 'full':
        start, end = torch.from_numpy(d.window[:, 0]).long(), torch.from_numpy(d.window[:, 1]).long()
        cond[:, :, -4:] = 0.
        for idx in range(bs):
            cond[idx, start[idx]:end[idx], TRAJ:] = 0
    if input_noise:
        cond[:, :, -4:] = 0.
    return (torch.permute(cond, (0, 2, 1)).unsqueeze(-2).contiguous(),
            torch.permute(clean, (0, 2, 1)).unsqueeze(-2).contiguous())


def alternate(sides, min_seconds, window=0.1):
    """{name: fn} -> {name: (ms per call, calls, least window's ms per call, greatest window's)}: the sides take turns in windows of about `window` seconds each (the calls per
    window are sized per side from one timed call, so a slow side does not stretch the run), every window closed by a
    synchronise, until each side has at least min_seconds."""
    chunk = {}
    for name, fn in sides.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        chunk[name] = max(1, min(1000, int(window / max(time.perf_counter() - t0, 1e-6))))
    total, calls, per_window = {k: 0.0 for k in sides}, {k: 0 for k in sides}, {k: [] for k in sides}
    while min(total.values()) < min_seconds:
        for name, fn in sides.items():
            t0 = time.perf_counter()
            for _ in range(chunk[name]):
                fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            total[name] += dt
            calls[name] += chunk[name]
            per_window[name].append(dt * 1e3 / chunk[name])
    return {k: (total[k] * 1e3 / calls[k], calls[k], min(per_window[k]), max(per_window[k])) for k in sides}


def decisions(B, T, bank):
    sched = M.PoseMaskSchedule(0, 'lower+upper+full', True, bank)
    random.seed(0)
    torch.manual_seed(0)
    np.random.seed(0)
    out = {'joints': sched.decide(0, B, T)}
    while len(out) < 5:
        d = sched.decide(1, B, T)
        out.setdefault(d.branch, d)
    return sched, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=64)
    ap.add_argument('--T', type=int, default=144)
    ap.add_argument('--step-T', type=int, default=143)
    ap.add_argument('--min-seconds', type=float, default=1.0)
    ap.add_argument('--prox-clips', type=int, default=500)
    ap.add_argument('--optimizer', choices=['torch', 'native'], default='torch')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'train_loop_timing.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_train_loop.py measures on the GPU; none is visible')
    dev, B, T = 'cuda:0', a.B, a.T
    rng = np.random.RandomState(0)
    masks = [(rng.rand(a.prox_clips * (T + 1), 25) > 0.2).astype(np.float64)]
    bank = M.ProxMaskBank(masks=masks, clip_len=T + 1, device=dev)
    # the reference's host array of the same clips: [n, clip_len, 294] float64
    import importlib.util
    spec = importlib.util.spec_from_file_location('train_masks_ref', os.path.join(ROOT, 'tests', 'train_masks_ref.py'))
    MR = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(MR)
    prox_host = np.stack([MR.vis_vector(w) for w in bank.bits_host])
    src = torch.randn(B, T, 294, device=dev)
    clean = torch.randn(B, T, 294, device=dev)
    sched, decs = decisions(B, T, bank)
    result = {'B': B, 'T': T, 'prox_clips': len(bank), 'prox_host_array_MB': prox_host.nbytes / 2 ** 20,
              'prox_device_words_MB': bank.bits_host.nbytes / 2 ** 20, 'min_seconds': a.min_seconds, 'branches': {},
              'device': torch.cuda.get_device_name(0)}
    for name, d in decs.items():
        if name == 'prox':                  # the check uses the decision's own clips; the timed side shuffles as the reference does
            ref = indexed_block(M.PoseMaskDecision('none'), src * torch.from_numpy(prox_host[d.vis_index]).float().to(dev)[:, 0:-1],
                                clean, prox_host, True)
        else:
            ref = indexed_block(d, src, clean, prox_host, True)
        got = sched.apply(d, src, clean)
        same = bool(torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]))
        if not same:
            raise SystemExit(f'branch {name}: the two sides differ')
        native = (lambda d=d: sched.apply(d, src, clean)) if name != 'prox' else \
            (lambda: sched.apply(M.PoseMaskDecision('prox', vis_index=bank.draw(B), zero_contact=True), src, clean))
        t = alternate({'native': native,
                       'indexed': lambda d=d: indexed_block(d, src, clean, prox_host, True)}, a.min_seconds)
        result['branches'][name] = {'native_ms': t['native'][0], 'indexed_ms': t['indexed'][0], 'native_calls': t['native'][1],
                                    'indexed_calls': t['indexed'][1], 'same_bits': same}
        print(f"{name:7s} native {t['native'][0]:8.4f} ms   indexed {t['indexed'][0]:8.4f} ms", flush=True)

    # ---- a whole PoseNet training step, for the share
    from rohm_amd.body_model import SMPLXLayer
    from rohm_amd.diffusion import gaussian_diffusion_posenet as gdp
    from rohm_amd.diffusion.respace import SpacedDiffusionPoseNet
    from rohm_amd.model.posenet import PoseNet
    from rohm_amd.utils.model_util import create_gaussian_diffusion

    class DS:
        pose_feat_dim, traj_feat_dim, body_feat_dim, joints_num = 272, 22, 294, 22
        Mean, Std = synth.synthetic_stats(0)

    class Args:
        noise_schedule, sigma_small = 'cosine', True
    Ts = a.step_T
    layer = SMPLXLayer.from_tensors(synth.synthetic_smplx_tensors(0)).to(dev)
    net = PoseNet(DS(), 294, latent_dim=512, ff_size=1024, num_layers=8, num_heads=4, dropout=0.1, traj_feat_dim=22,
                  body_model_path=layer, device=dev, weight_loss_rec_repr_full_body=1.0, weight_loss_repr_foot_contact_mse=1.0,
                  weight_loss_joint_pos_global=100.0, weight_loss_joint_vel_global=1000.0, weight_loss_foot_skating=0.1,
                  start_skating_loss_epoch=1000)
    net.load_state_dict(synth.posenet_state_dict(0), strict=False)
    net = net.to(dev).train()
    diff = create_gaussian_diffusion(Args, gdp, SpacedDiffusionPoseNet, 1000, '', device=dev)
    from rohm_amd.optim import AdamW as NativeAdamW
    trainable = [p for p in net.parameters() if p.requires_grad]
    opts = {'torch': torch.optim.AdamW(trainable, lr=1e-4)}
    if a.optimizer == 'native':
        opts['native'] = NativeAdamW(trainable, lr=1e-4)
    opt = opts[a.optimizer]
    rows = synth.plausible_motion(3, B, Ts, DS.Mean, DS.Std)[:, :, 0].permute(0, 2, 1).contiguous().to(dev)
    noisy = (rows + 0.05 * torch.randn_like(rows)).contiguous()
    bank_s = M.ProxMaskBank(masks=[masks[0][:a.prox_clips * (Ts + 1)]], clip_len=Ts + 1, device=dev)
    sched_s = M.PoseMaskSchedule(0, 'lower+upper+full', True, bank_s)

    def step(with_masks, opt=opt):
        batch = {'motion_repr_clean': rows, 'motion_repr_noisy': noisy}
        if with_masks:
            sched_s(batch, 1)
        else:
            batch['cond'], batch['motion_repr_clean'] = cond_fixed, clean_fixed
        opt.zero_grad()
        t = torch.from_numpy(np.random.choice(1000, size=(B,))).long().to(dev)
        losses, _ = diff.training_losses(model=net, batch=batch, t=t, noise=None)
        losses['loss'].backward()
        opt.step()
    cond_fixed, clean_fixed = sched_s.apply(sched_s.decide(1, B, Ts), noisy, rows)
    t = alternate({'step': lambda: step(True), 'step_without_mask_block': lambda: step(False)}, a.min_seconds)
    result['posenet_step'] = {'T': Ts, 'layers': 8, 'step_ms': t['step'][0], 'step_without_mask_block_ms': t['step_without_mask_block'][0],
                              'calls': t['step'][1]}
    result['posenet_step']['optimizer'] = a.optimizer
    print(f"PoseNet step at T = {Ts}: {t['step'][0]:.3f} ms with the mask block, {t['step_without_mask_block'][0]:.3f} ms without",
          flush=True)
    if a.optimizer == 'native':
        # The same whole step under each optimiser, taking turns.  Both step the SAME parameter tensors, each with its own
        # moments: fine for a timing (the work per step does not depend on the values), meaningless as a training run.
        t = alternate({k: (lambda o=o: step(True, o)) for k, o in opts.items()}, a.min_seconds)
        result['posenet_step_by_optimizer'] = {k: {'step_ms': v[0], 'calls': v[1], 'window_ms_min': v[2], 'window_ms_max': v[3]}
                                               for k, v in t.items()}
        print('PoseNet step by optimiser: ' + ', '.join(f'{k} {v[0]:.3f} ms [{v[2]:.3f}, {v[3]:.3f}]' for k, v in t.items()),
              flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
