"""RoHM's training loops (train/training_loop_posenet.py, train/training_loop_trajnet.py) on the native pieces: device batches,
the mask schedules of `rohm_amd.train.masks`, the native `training_losses`, and AdamW: torch's by default, or the native
`rohm_amd.optim.AdamW` (one fused pass, optional gradient-norm clipping on the device) with `args.optimizer = 'native'` and
`args.max_grad_norm`.

The classes keep the reference's constructor arguments and methods (`run_loop`, `run_step`, `forward_backward`, `save`,
`ckpt_file_name`).  A loader is either a `DataloaderAMASS`, iterated with `batches()`, or any iterable of dict batches that has
`len()` and a `.dataset` with `clip_len` and `traj_feat_dim`.  Stated differences from the reference:
  * PoseNet's eval report is the true mean over the test batches (the reference's `eval_losses[key] += eval_losses[key]` doubles
    the last batch's value instead of accumulating);
  * checkpoints are written with plain `torch.save(model.state_dict(), path)`, no blobfile;
  * `writer` may be None; `JsonlWriter` stands in for tensorboardX's SummaryWriter;
  * nothing reads a loss on the host except at the log / eval / save steps.
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch
from torch.optim import AdamW

from ..data_loaders.dataloader_amass import DataloaderAMASS
from .masks import PoseMaskSchedule, ProxMaskBank, TrajMaskSchedule


class JsonlWriter:
    """`add_scalar(tag, value, step)` as one JSON line per call in <log_dir>/scalars.jsonl."""

    def __init__(self, log_dir):
        os.makedirs(log_dir, exist_ok=True)
        self.path = os.path.join(log_dir, 'scalars.jsonl')
        self._f = open(self.path, 'a')

    def add_scalar(self, tag, value, step):
        self._f.write(json.dumps({'tag': tag, 'value': float(value), 'step': int(step)}) + '\n')
        self._f.flush()

    def close(self):
        self._f.close()


class _Loader:
    """One face for the two kinds of loader: len() in batches, .dataset, iteration over device dict batches."""

    def __init__(self, loader, batch_size, shuffle, device, generator=None):
        self.loader, self.batch_size, self.shuffle, self.device, self.generator = loader, batch_size, shuffle, device, generator
        self.native = isinstance(loader, DataloaderAMASS)
        self.dataset = loader if self.native else loader.dataset

    def __len__(self):
        if self.native:
            return (len(self.loader) + self.batch_size - 1) // self.batch_size
        return len(self.loader)

    def __iter__(self):
        if self.native:
            yield from self.loader.batches(self.batch_size, shuffle=self.shuffle, drop_last=False, generator=self.generator)
            return
        for batch in self.loader:
            yield {k: torch.as_tensor(v).to(self.device) for k, v in batch.items()}


class _TrainLoop:
    def __init__(self, args, writer, model, diffusion_train, diffusion_eval, timestep_respacing_eval, train_dataloader,
                 test_dataloader, logdir, logger, device, generator, smplx_model):
        self.args, self.writer, self.model = args, writer, model
        self.diffusion_train, self.diffusion_eval = diffusion_train, diffusion_eval
        self.batch_size, self.lr = args.batch_size, args.lr
        self.log_interval, self.save_interval = args.log_interval, args.save_interval
        self.weight_decay = args.weight_decay
        self.timestep_respacing_eval = timestep_respacing_eval
        self.device = torch.device(device)
        self.train_dataloader = _Loader(train_dataloader, self.batch_size, True, self.device, generator)
        self.test_dataloader = _Loader(test_dataloader, self.batch_size, False, self.device) if test_dataloader is not None else None
        self.smplx_neutral = smplx_model
        self.step = 0
        self.num_steps = args.num_steps
        self.num_epochs = self.num_steps // len(self.train_dataloader) + 1
        self.save_dir, self.logger = logdir, logger
        self.opt = self._make_optimizer([p for p in self.model.parameters() if p.requires_grad])
        # UniformSampler (diffusion/resample.py): every timestep has weight 1
        self._p = np.ones([diffusion_train.num_timesteps]) / diffusion_train.num_timesteps

    def _make_optimizer(self, params):
        """args.optimizer: 'torch' (the default: torch.optim.AdamW, as the reference) or 'native' (rohm_amd.optim.AdamW);
        args.max_grad_norm: clip the global gradient norm, native only."""
        kind = getattr(self.args, 'optimizer', 'torch')
        max_grad_norm = getattr(self.args, 'max_grad_norm', None)
        if kind == 'torch':
            if max_grad_norm is not None:
                raise ValueError("max_grad_norm needs optimizer='native': the torch optimiser of the loop does not clip")
            return AdamW(params, lr=self.lr, weight_decay=self.weight_decay)
        if kind != 'native':
            raise ValueError(f"optimizer must be 'torch' or 'native', got {kind!r}")
        from ..optim import AdamW as NativeAdamW
        return NativeAdamW(params, lr=self.lr, weight_decay=self.weight_decay, max_grad_norm=max_grad_norm)

    # -- the pieces of a step ----------------------------------------------------------------------------------------------------
    def sample_timesteps(self, batch_size):
        """UniformSampler.sample: indices from np.random.choice, importance weights 1 / (len(p) * p[i])."""
        p = self._p
        indices_np = np.random.choice(len(p), size=(batch_size,), p=p)
        t = torch.from_numpy(indices_np).long().to(self.device)
        weights = torch.from_numpy(1 / (len(p) * p[indices_np])).float().to(self.device)
        return t, weights

    def run_step(self, batch):
        losses = self.forward_backward(batch)
        self.opt.step()
        return losses

    def _info(self, msg):
        if self.logger is not None:
            self.logger.info(msg)

    def _report(self, kind, epoch, losses):
        """The reference's log lines; the only place a loss is read on the host."""
        for key in losses.keys():
            value = losses[key].item()
            if self.writer is not None:
                self.writer.add_scalar('{}/{}'.format('train' if kind == 'train' else 'eval', key), value, self.step)
            print_str = '[Step {:d}/ Epoch {:d}] [{}]  {}: {:.10f}'.format(self.step, epoch, kind, key, value)
            self._info(print_str)
            print(print_str)

    def _after_step(self, epoch, train_losses):
        if self.step % self.log_interval == 0 and self.step > 0:
            self._report('train', epoch, train_losses)
            if self.test_dataloader is not None:
                self.model.eval()
                self._report('test', epoch, self.evaluate(epoch))
                self.model.train()
        if self.step % self.save_interval == 0 and self.step > 0:
            self.save()
        self.step += 1

    def _mean_eval(self, per_batch):
        """Mean over the test batches of every reported loss, accumulated on the device."""
        total, n = {}, 0
        for losses in per_batch:
            for key, v in losses.items():
                total[key] = v.detach().clone() if n == 0 else total[key] + v.detach()
            n += 1
        return {k: v / n for k, v in total.items()}

    def ckpt_file_name(self):
        return f"model{(self.step):09d}.pt"

    def save(self):
        os.makedirs(self.save_dir, exist_ok=True)
        torch.save(self.model.state_dict(), os.path.join(self.save_dir, self.ckpt_file_name()))
        self._info('[*] model saved\n')


class TrainLoopPoseNet(_TrainLoop):
    """train/training_loop_posenet.py.  prox_bank: a ProxMaskBank; None reads `<parent of args.dataset_root>/PROX/mask_joint` when
    the schedule first needs it (the reference reads it at the start of run_loop)."""

    def __init__(self, args, writer, model, diffusion_train, diffusion_eval, timestep_respacing_eval, input_noise,
                 train_dataloader, test_dataloader, logdir, logger, start_prox_mask_epoch, mask_scheme, device='cuda',
                 prox_bank=None, generator=None, smplx_model=None):
        super().__init__(args, writer, model, diffusion_train, diffusion_eval, timestep_respacing_eval, train_dataloader,
                         test_dataloader, logdir, logger, device, generator, smplx_model)
        self.input_noise, self.start_prox_mask_epoch, self.mask_scheme = input_noise, start_prox_mask_epoch, mask_scheme
        self.schedule = PoseMaskSchedule(start_prox_mask_epoch, mask_scheme, input_noise, prox_bank)

    def _load_prox_bank(self):
        print('[INFO] loading PROX joint masks...')
        all_dataset_root = '/'.join(self.args.dataset_root.split('/')[0:-1])
        bank = ProxMaskBank(all_dataset_root, self.train_dataloader.dataset.clip_len, self.device)
        print('[INFO] prox masks loaded, get {} prox mask clips in total.'.format(len(bank)))
        return bank

    def run_loop(self):
        if self.schedule.prox_bank is None and self.num_epochs - 1 > self.start_prox_mask_epoch:
            self.schedule.prox_bank = self._load_prox_bank()
        for epoch in range(self.num_epochs):
            self.model.train()
            for batch in self.train_dataloader:
                self.schedule(batch, epoch)
                train_losses = self.run_step(batch)
                self._after_step(epoch, train_losses)

    def evaluate(self, epoch):
        def per_batch():
            for test_batch in self.test_dataloader:
                self.schedule(test_batch, epoch, eval_block=True)
                shape = list(test_batch['motion_repr_clean'].shape)
                with torch.no_grad():
                    losses, _ = self.diffusion_eval.eval_losses(model=self.model, batch=test_batch, shape=shape, progress=False,
                                                                clip_denoised=False, cur_epoch=epoch,
                                                                timestep_respacing=self.timestep_respacing_eval,
                                                                smplx_model=self.smplx_neutral, compute_loss=True)
                yield losses
        return self._mean_eval(per_batch())

    def forward_backward(self, batch):
        self.opt.zero_grad()
        t, weights = self.sample_timesteps(batch['motion_repr_clean'].shape[0])
        losses, _ = self.diffusion_train.training_losses(model=self.model, batch=batch, t=t, noise=None,
                                                         smplx_model=self.smplx_neutral)
        loss = (losses["loss"] * weights).mean()
        loss.backward()
        return losses


class TrainLoopTrajNet(_TrainLoop):
    """train/training_loop_trajnet.py."""

    def __init__(self, args, writer, model, diffusion_train, diffusion_eval, timestep_respacing_eval, start_infill_epoch,
                 max_infill_ratio, mask_prob, train_dataloader, test_dataloader, logdir, logger, device='cuda', generator=None,
                 smplx_model=None):
        super().__init__(args, writer, model, diffusion_train, diffusion_eval, timestep_respacing_eval, train_dataloader,
                         test_dataloader, logdir, logger, device, generator, smplx_model)
        self.start_infill_epoch, self.mask_prob, self.max_infill_ratio = start_infill_epoch, mask_prob, max_infill_ratio
        self.schedule = TrajMaskSchedule(start_infill_epoch, mask_prob, max_infill_ratio)

    def run_loop(self):
        traj_feat_dim = self.train_dataloader.dataset.traj_feat_dim
        for epoch in range(self.num_epochs):
            self.model.train()
            for batch in self.train_dataloader:
                self.schedule(batch, epoch, traj_feat_dim)
                train_losses = self.run_step(batch)
                self._after_step(epoch, train_losses)

    def evaluate(self, epoch):
        traj_feat_dim = self.train_dataloader.dataset.traj_feat_dim

        def per_batch():
            for test_batch in self.test_dataloader:
                shape = list(test_batch['motion_repr_clean'][:, :, 0:traj_feat_dim].shape)
                with torch.no_grad():
                    losses, _ = self.diffusion_eval.eval_losses(model=self.model, batch=test_batch, shape=shape, progress=False,
                                                                clip_denoised=False, cur_epoch=epoch,
                                                                timestep_respacing=self.timestep_respacing_eval,
                                                                smplx_model=self.smplx_neutral, compute_loss=True)
                yield losses
        return self._mean_eval(per_batch())

    def forward_backward(self, batch):
        self.opt.zero_grad()
        t, weights = self.sample_timesteps(batch['motion_repr_clean'].shape[0])
        losses = self.diffusion_train.training_losses(model=self.model, batch=batch, t=t, noise=None,
                                                      traj_feat_dim=self.train_dataloader.dataset.traj_feat_dim,
                                                      smplx_model=self.smplx_neutral)
        loss = (losses["loss"] * weights).mean()
        loss.backward()
        return losses
