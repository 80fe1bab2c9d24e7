"""`python -m rohm_amd.train posenet|trajnet --config cfg.yaml [--key value ...]`: the reference's train_posenet.py /
train_trajnet.py on the native loader, models, losses and loops.

The arguments and their defaults are those of train_posenet.py:26-69 and train_trajnet.py:28-76.  A config file is the flat
`key: value  # comment` text of cfg_files/train_cfg/*.yaml, read by `read_config` (no configargparse, no PyYAML); command-line
values override it.  Two arguments are the package's own: `--optimizer torch|native` (default torch: torch.optim.AdamW as the
reference; native: rohm_amd.optim.AdamW, one fused HIP pass over all parameters) and `--max_grad_norm X` (default none; native
only: clip the global gradient norm on the device).  Out of scope, as in the rest of the package's training path: mixed
precision, multi-GPU training, and the shuffle order or hidden seed draws of the reference's DataLoader.
"""
from __future__ import annotations

import argparse
import logging
import os
import random
import sys

import torch

_bool = lambda x: str(x).lower() in ['true', '1']      # noqa: E731  (the drivers' own rule)
_opt_float = lambda x: None if str(x).lower() in ['none', ''] else float(x)      # noqa: E731


COMMON = [
    ('device', 0, int),
    ('noise_schedule', 'cosine', str), ('timestep_respacing_eval', '', str), ('sigma_small', True, _bool),
    ('body_model_path', 'body_models/smplx_model', str),
    ('dataset_root', '/mnt/hdd/diffusion_mocap_datasets/AMASS_smplx_preprocessed', str),
    ('clip_len', 145, int), ('load_pretrained_model', False, _bool), ('pretrained_model_path', '', str),
    ('input_noise', True, _bool), ('noise_std_smplx_global_rot', 3.0, float), ('noise_std_smplx_body_rot', 2.0, float),
    ('noise_std_smplx_betas', 0.2, float),
    ('debug', False, _bool), ('save_dir', 'runs', str), ('lr', 1e-4, float), ('weight_decay', 0.0, float),
    ('log_interval', 25000, int), ('save_interval', 25000, int), ('num_steps', 1000000_000, int),
    ('optimizer', 'torch', str), ('max_grad_norm', None, _opt_float),
]
POSENET = COMMON + [
    ('diffusion_steps', 1000, int), ('task', 'pose', str), ('noise_std_smplx_trans', 0.01, float),
    ('weight_loss_rec_repr_full_body', 1.0, float), ('weight_loss_repr_foot_contact_mse', 1.0, float),
    ('weight_loss_joint_pos_global', 100.0, float), ('weight_loss_joint_vel_global', 1000.0, float),
    ('weight_loss_joint_smooth', 0.0, float), ('start_skating_loss_epoch', 1000, int), ('weight_loss_foot_skating', 0.0, float),
    ('batch_size', 32, int), ('start_prox_mask_epoch', 500, int), ('mask_scheme', 'lower', str),
]
TRAJNET = COMMON + [
    ('diffusion_steps', 100, int), ('task', 'traj', str), ('noise_std_smplx_trans', 0.02, float),
    ('repr_abs_only', True, _bool), ('trajcontrol', False, _bool), ('load_pretrained_backbone', False, _bool),
    ('pretrained_backbone_path', '', str),
    ('weight_loss_root_rec_repr', 1.0, float), ('weight_loss_root_pos_global', 100.0, float),
    ('weight_loss_root_vel_global', 1000.0, float), ('weight_loss_root_rot_vel_from_abs_traj', 1.0, float),
    ('weight_loss_root_smplx_transl_vel', 1000.0, float), ('weight_loss_root_smplx_rot_vel', 1.0, float),
    ('weight_loss_root_smooth', 0.0, float), ('weight_loss_root_rot_cos_smooth_from_abs_traj', 0.0, float),
    ('batch_size', 64, int), ('max_infill_ratio', 0.1, float), ('mask_prob', 0.4, float),
    ('start_infill_epoch', 100000000000000000000, int),
]
SPECS = {'posenet': POSENET, 'trajnet': TRAJNET}
CHOICES = {'noise_schedule': ['linear', 'cosine'], 'task': ['traj', 'pose'], 'optimizer': ['torch', 'native'],
           'mask_scheme': ['lower', 'lower+upper', 'lower+full', 'lower+upper+full']}
TRAIN_DATASETS = ['HumanEva', 'HDM05', 'MoSh', 'Transitions', 'ACCAD', 'BMLhandball', 'BMLmovi', 'BMLrub', 'CMU', 'DFaust',
                  'Eyes_Japan_Dataset', 'PosePrior', 'SSM', 'GRAB', 'SOMA']
TEST_DATASETS = ['TCDHands', 'TotalCapture', 'SFU']


def _strip_comment(text):
    quote = None
    for i, ch in enumerate(text):
        if quote:
            quote = None if ch == quote else quote
        elif ch in '\'"':
            quote = ch
        elif ch == '#':
            return text[:i]
    return text


def read_config(path):
    """A flat `key: value  # comment` file -> {key: value string}; quotes around a value are dropped."""
    out = {}
    with open(path) as f:
        for n, line in enumerate(f, start=1):
            line = _strip_comment(line).strip()
            if not line:
                continue
            key, sep, value = line.partition(':')
            if not sep or not key.strip():
                raise ValueError(f'{path}:{n}: expected `key: value`, got {line!r}')
            value = value.strip()
            if len(value) >= 2 and value[0] == value[-1] and value[0] in '\'"':
                value = value[1:-1]
            out[key.strip()] = value
    return out


def parse_args(which, argv):
    """Namespace of the driver's arguments: defaults, then the config file's values, then the command line's."""
    spec = SPECS[which]
    pre = argparse.ArgumentParser(add_help=False)
    pre.add_argument('--config', default='')
    known, _ = pre.parse_known_args(argv)
    parser = argparse.ArgumentParser(prog=f'python -m rohm_amd.train {which}', description='RoHM training on an AMD GPU')
    parser.add_argument('--config', default='', help='config file path')
    for name, default, typ in spec:
        parser.add_argument('--' + name, default=default, type=typ, choices=CHOICES.get(name))
    if known.config:
        types = {name: typ for name, _, typ in spec}
        cfg = read_config(known.config)
        unknown = sorted(set(cfg) - set(types))
        if unknown:
            raise ValueError(f'{known.config}: unknown settings {unknown}')
        values = {k: types[k](v) for k, v in cfg.items()}
        for k, v in values.items():
            if k in CHOICES and v not in CHOICES[k]:
                raise ValueError(f'{known.config}: {k} must be one of {CHOICES[k]}, got {v!r}')
        parser.set_defaults(**values)
    args = parser.parse_args(argv)
    if args.max_grad_norm is not None and args.optimizer != 'native':
        raise ValueError("max_grad_norm needs optimizer = native: the torch optimiser of the loops does not clip")
    return args


def prepare_trajcontrol(model, backbone_state_dict=None):
    """train_trajnet.py:149-175: load the pretrained backbone non-strictly and copy its `diff*` weights to the control branch
    ('controlnet.control' + key[4:]), then freeze everything but `controlnet.*` (the frozen blocks go to eval mode)."""
    if backbone_state_dict is not None:
        model.load_state_dict(backbone_state_dict, strict=False)
        copy = {'controlnet.control' + key[4:]: value for key, value in backbone_state_dict.items()
                if key.split('.')[0].split('_')[0] == 'diff'}
        model.load_state_dict(copy, strict=False)
    for name, param in model.named_parameters():
        param.requires_grad = name.split('.')[0].split('_')[0] == 'controlnet'
    for name, layer in model.named_modules():
        if name.split('.')[0].split('_')[0] in ['cond', 'diff', 'time']:
            layer.eval()
    return model


def get_logger(logdir):
    os.makedirs(logdir, exist_ok=True)
    logger = logging.getLogger('rohm_amd.train.' + logdir)
    logger.setLevel(logging.INFO)
    handler = logging.FileHandler(os.path.join(logdir, 'train.log'))
    handler.setFormatter(logging.Formatter('%(asctime)s %(message)s'))
    logger.addHandler(handler)
    return logger


def _datasets(args, device, logdir):
    from ..data_loaders.dataloader_amass import DataloaderAMASS
    train_sets, test_sets = (['HumanEva'], ['TCDHands']) if args.debug else (TRAIN_DATASETS, TEST_DATASETS)
    kw = dict(preprocessed_amass_root=args.dataset_root, body_model_path=args.body_model_path,
              repr_abs_only=getattr(args, 'repr_abs_only', False), input_noise=args.input_noise,
              noise_std_smplx_global_rot=args.noise_std_smplx_global_rot, noise_std_smplx_body_rot=args.noise_std_smplx_body_rot,
              noise_std_smplx_trans=args.noise_std_smplx_trans, noise_std_smplx_betas=args.noise_std_smplx_betas,
              task=args.task, clip_len=args.clip_len, logdir=logdir, device=device)
    print("creating data loader...")
    return (DataloaderAMASS(split='train', amass_datasets=train_sets, **kw),
            DataloaderAMASS(split='test', spacing=2, amass_datasets=test_sets, **kw))


def _load(path):
    return torch.load(path, map_location=lambda storage, loc: storage)


def main_posenet(args, writer, logdir, logger):
    from ..diffusion import gaussian_diffusion_posenet
    from ..diffusion.respace import SpacedDiffusionPoseNet
    from ..model.posenet import PoseNet
    from ..utils.model_util import create_gaussian_diffusion
    from .loops import TrainLoopPoseNet
    device = f'cuda:{args.device}'
    train_dataset, test_dataset = _datasets(args, device, logdir)
    print("creating model and diffusion...")
    model = PoseNet(dataset=train_dataset, body_feat_dim=train_dataset.body_feat_dim, latent_dim=512, ff_size=1024, num_layers=8,
                    num_heads=4, dropout=0.1, activation="gelu", body_model_path=args.body_model_path, device=device,
                    traj_feat_dim=train_dataset.traj_feat_dim,
                    weight_loss_rec_repr_full_body=args.weight_loss_rec_repr_full_body,
                    weight_loss_repr_foot_contact_mse=args.weight_loss_repr_foot_contact_mse,
                    weight_loss_joint_pos_global=args.weight_loss_joint_pos_global,
                    weight_loss_joint_vel_global=args.weight_loss_joint_vel_global,
                    weight_loss_joint_smooth=args.weight_loss_joint_smooth,
                    weight_loss_foot_skating=args.weight_loss_foot_skating,
                    start_skating_loss_epoch=args.start_skating_loss_epoch).to(device)
    if args.load_pretrained_model:
        model.load_state_dict(_load(args.pretrained_model_path))
        print('loaded checkpoint from {}'.format(args.pretrained_model_path))
    make = lambda: create_gaussian_diffusion(args, gd=gaussian_diffusion_posenet, return_class=SpacedDiffusionPoseNet,  # noqa: E731
                                             num_diffusion_timesteps=args.diffusion_steps,
                                             timestep_respacing=args.timestep_respacing_eval, device=device)
    print("Training...")
    TrainLoopPoseNet(args, writer=writer, model=model, diffusion_train=make(), diffusion_eval=make(),
                     timestep_respacing_eval=args.timestep_respacing_eval, train_dataloader=train_dataset,
                     test_dataloader=test_dataset, logdir=logdir, logger=logger,
                     start_prox_mask_epoch=args.start_prox_mask_epoch, mask_scheme=args.mask_scheme,
                     input_noise=args.input_noise, device=device).run_loop()


def main_trajnet(args, writer, logdir, logger):
    from ..diffusion import gaussian_diffusion_trajnet
    from ..diffusion.respace import SpacedDiffusionTrajNet
    from ..model.posenet import _make_body_model
    from ..model.trajnet import TrajNet
    from ..utils.model_util import create_gaussian_diffusion
    from .loops import TrainLoopTrajNet
    device = f'cuda:{args.device}'
    train_dataset, test_dataset = _datasets(args, device, logdir)
    print("creating model and diffusion...")
    weights = {k: v for k, v in vars(args).items() if k.startswith('weight_loss_root_')}
    model = TrajNet(time_dim=32, mid_dim=512, cond_dim=train_dataset.traj_feat_dim, traj_feat_dim=train_dataset.traj_feat_dim,
                    trajcontrol=args.trajcontrol, device=device, dataset=train_dataset, repr_abs_only=args.repr_abs_only,
                    **weights).to(device)
    if args.load_pretrained_model:
        model.load_state_dict(_load(args.pretrained_model_path))
        print('loaded checkpoint from {}'.format(args.pretrained_model_path))
    if args.trajcontrol:
        backbone = None
        if args.load_pretrained_backbone:
            if args.load_pretrained_model:
                raise SystemExit('[ERROR] for TrajControl finetune, cannot set both load_pretrained_backbone and '
                                 'load_pretrained_model to True!')
            backbone = _load(args.pretrained_backbone_path)
            print('loaded pretrained backbone from {}'.format(args.pretrained_backbone_path))
        prepare_trajcontrol(model, backbone)
    make = lambda respacing: create_gaussian_diffusion(args, gd=gaussian_diffusion_trajnet,  # noqa: E731
                                                       return_class=SpacedDiffusionTrajNet,
                                                       num_diffusion_timesteps=args.diffusion_steps,
                                                       timestep_respacing=respacing, device=device)
    print("Training...")
    TrainLoopTrajNet(args, writer=writer, model=model, diffusion_train=make(''), diffusion_eval=make(args.timestep_respacing_eval),
                     timestep_respacing_eval=args.timestep_respacing_eval, start_infill_epoch=args.start_infill_epoch,
                     max_infill_ratio=args.max_infill_ratio, mask_prob=args.mask_prob, train_dataloader=train_dataset,
                     test_dataloader=test_dataset, logdir=logdir, logger=logger, device=device,
                     smplx_model=_make_body_model(args.body_model_path, device)).run_loop()


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv or argv[0] not in SPECS:
        raise SystemExit('usage: python -m rohm_amd.train posenet|trajnet --config cfg.yaml [--key value ...]')
    which, args = argv[0], parse_args(argv[0], argv[1:])
    from .loops import JsonlWriter
    run_id = random.randint(1, 100000)
    logdir = os.path.join(args.save_dir, str(run_id))
    writer = JsonlWriter(logdir)
    print('RUNDIR: {}'.format(logdir))
    sys.stdout.flush()
    logger = get_logger(logdir)
    logger.info('Let the games begin')
    with open(os.path.join(logdir, 'config.yaml'), 'w') as f:
        for k, v in sorted(vars(args).items()):
            f.write(f'{k}: {v}\n')
    {'posenet': main_posenet, 'trajnet': main_trajnet}[which](args, writer, logdir, logger)
    writer.close()


if __name__ == '__main__':
    main()
