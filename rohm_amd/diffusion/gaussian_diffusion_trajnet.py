"""Drop-in for RoHM's `diffusion/gaussian_diffusion_trajnet.py` (module object passed as `gd=`)."""
import torch

from .ddpm import (DDPMSampler, LossType, ModelMeanType, ModelVarType, _extract_into_tensor,  # noqa: F401
                   betas_for_alpha_bar, get_named_beta_schedule)


class GaussianDiffusionTrajNet(DDPMSampler):
    """TrajNet diffusion: native 100-step cosine schedule, no guidance
    (gaussian_diffusion_trajnet.py:440-466)."""

    supports_guidance = False

    def eval_losses(self, model, batch, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                    device=None, progress=False, skip_timesteps=0, init_data=None, randomize_class=False,
                    cond_fn_with_grad=False, cond_grad_weight=1.0, dump_steps=None, const_noise=False,
                    cur_epoch=0, timestep_respacing='', compute_loss=True, smplx_model=None):
        """Entry point used by the drivers (gaussian_diffusion_trajnet.py:878-915) -> (loss report or None, x0 [B, T, 13])."""
        return self._eval(model, batch, shape, progress, clip_denoised, cond_fn_with_grad, None, False,
                          timestep_respacing, compute_loss, smplx_model)

    def training_losses(self, model, batch, t, noise=None, traj_feat_dim=4, smplx_model=None):
        """gaussian_diffusion_trajnet.py:857-875: batch['x_t'] = q_sample(motion_repr_clean[:, :, :traj_feat_dim], t, noise); the
        model's train-mode forward (differentiable when the module is in train mode with grad enabled);
        compute_losses_with_smpl -> loss_dict.  With repr_abs_only the drivers' dataset hands over motion_repr_clean with the
        absolute-trajectory channels first, so the slice is taken literally as in the reference."""
        from ..model.trajnet import TrajNet
        net = getattr(model, 'model', model)
        if not isinstance(net, TrajNet):
            return super().training_losses(model, batch, t, noise=noise, smplx_model=smplx_model)
        x_start = batch['motion_repr_clean'][:, :, :traj_feat_dim]
        if noise is None:
            noise = torch.randn_like(x_start)
        batch['x_t'] = self.q_sample(x_start, t, noise=noise)
        model_output = net(batch, self._scale_timesteps(t))
        return net.compute_losses_with_smpl(batch, model_output, smplx_model)
