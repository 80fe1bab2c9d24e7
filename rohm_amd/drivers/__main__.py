"""`python -m rohm_amd.drivers amass_full|prox_egobody|posenet|trajnet|track [--config cfg.yaml] [--key value ...]`: the reference's
test_amass_full.py / test_prox_egobody.py / test_posenet.py / test_trajnet.py on the native loaders, networks, samplers and
result tails (rohm_amd.drivers.results).

The arguments, their defaults and types are those of test_amass_full.py:26-71, test_prox_egobody.py:27-66, test_posenet.py:22-54
and test_trajnet.py:18-50; booleans follow the drivers' own 'true' / '1' rule.  A config file is the flat `key: value  # comment`
text of cfg_files/test_cfg/*.yaml (rohm_amd.train.__main__.read_config); command-line values override it; a setting the driver
does not have is an error.  The package's own arguments: `--rohm_root` / `--floor_heights` (prox_egobody: the floor tables, as in
rohm_amd.evaluation), `--eval_noise_root` (amass_full: the directory of smplx_noise_level_{k}.pkl, default data/eval_noise_smplx),
`--save_interval N` (also write the pickle after every N-th batch; default 0: once, after the last batch) and `--evaluate` (print the
evaluation lines straight from the device results).  Out of scope: sharding a driver over several GPUs (rohm_amd.sharding does that
from Python), the open3d viewers (`--visualize` is accepted and prints one line; pictures come from `rohm_amd.evaluation --render`) and the
reference's DataLoader worker processes.

`track` has no script behind it: it is `prox_egobody` on a generic track file (rohm_amd.data_loaders.track) -- `--track file.npz`
instead of `--dataset`, `--init_root`, `--dataset_root`, `--recording_name`, `--rohm_root` and `--floor_heights`, plus `--tail
cover|drop` and `--max_gap SECONDS`.
"""
from __future__ import annotations

import argparse
import os
import pickle
import random
import sys

import numpy as np
import torch

from ..train.__main__ import TEST_DATASETS, _bool, _load, read_config

_HEAD = [('device', 0, int), ('seed', 0, int)]
_SCHEDULE = [('noise_schedule', 'cosine', str), ('timestep_respacing_eval', '', str), ('sigma_small', True, _bool)]
_CHECKPOINTS = [('clip_len', 145, int), ('repr_abs_only', True, _bool),
                ('model_path_trajnet', '../diffusion_mocap/runs_try/79530/model000450000.pt', str),
                ('model_path_trajnet_control', '../diffusion_mocap/runs_try/65648/model000400000.pt', str),
                ('model_path_posenet', '../diffusion_mocap/runs_try/54359/model000200000.pt', str)]
_ITER = [('sample_iter', 2, int)]
_AMASS_ROOT = '/mnt/hdd/diffusion_mocap_datasets/AMASS_smplx_preprocessed'
AMASS_FULL = _HEAD + [('diffusion_steps_posenet', 1000, int), ('diffusion_steps_trajnet', 100, int)] + _SCHEDULE + [
    ('body_model_path', 'body_models/smplx_model', str), ('dataset_root', _AMASS_ROOT, str)] + _CHECKPOINTS + [
    ('input_noise', True, _bool), ('noise_std_smplx_global_rot', 3.0, float), ('noise_std_smplx_body_rot', 3.0, float),
    ('noise_std_smplx_trans', 0.03, float), ('noise_std_smplx_betas', 0.1, float), ('load_noise', True, _bool),
    ('load_noise_level', 3, int),
    ('batch_size', 32, int), ('cond_fn_with_grad', True, _bool), ('infill_traj', False, _bool), ('traj_mask_ratio', 0.1, float),
    ('mask_scheme', 'full', str), ('save_root', 'test_results/results_amass_full', str)] + _ITER + [
    ('iter2_cond_noisy_traj', True, _bool), ('iter2_cond_noisy_pose', True, _bool), ('early_stop', False, _bool)]
PROX_EGOBODY = _HEAD + [('diffusion_steps_posenet', 1000, int), ('diffusion_steps_trajnet', 100, int)] + _SCHEDULE + [
    ('body_model_path', 'body_models/smplx_model', str), ('dataset', 'egobody', str), ('dataset_root', '/mnt/ssd/egobody_release', str),
    ('init_root', 'data/init_motions/init_prox_rgb', str)] + _CHECKPOINTS + [
    ('batch_size', 20, int), ('cond_fn_with_grad', True, _bool), ('save_root', 'test_results/results_egobody', str)] + _ITER + [
    ('iter2_cond_noisy_traj', False, _bool), ('iter2_cond_noisy_pose', False, _bool), ('early_stop', True, _bool),
    ('window_size', 2, int), ('recording_name', 'recording_20211004_S12_S20_01', str), ('use_scene_floor_height', True, _bool)]
POSENET = _HEAD + [('diffusion_steps', 1000, int)] + _SCHEDULE + [
    ('body_model_path', 'body_models/smplx_model', str), ('dataset_root', _AMASS_ROOT, str), ('task', 'pose', str),
    ('clip_len', 145, int), ('model_path', 'checkpoints/posenet_checkpoint/model000200000.pt', str),
    ('input_noise', True, _bool), ('noise_std_smplx_global_rot', 3.0, float), ('noise_std_smplx_body_rot', 2.0, float),
    ('noise_std_smplx_trans', 0.01, float), ('noise_std_smplx_betas', 0.2, float),
    ('batch_size', 32, int), ('cond_fn_with_grad', False, _bool), ('mask_scheme', 'lower', str), ('visualize', True, _bool),
    ('vis_interval', 50, int), ('save_results', False, _bool)]
TRAJNET = _HEAD + [('diffusion_steps', 100, int)] + _SCHEDULE + [
    ('body_model_path', 'body_models/smplx_model', str), ('dataset_root', _AMASS_ROOT, str), ('task', 'traj', str),
    ('clip_len', 145, int), ('repr_abs_only', True, _bool), ('trajcontrol', False, _bool),
    ('model_path', 'checkpoints/trajnet_checkpoint/model000450000.pt', str),
    ('input_noise', True, _bool), ('noise_std_smplx_global_rot', 1.0, float), ('noise_std_smplx_body_rot', 1.0, float),
    ('noise_std_smplx_trans', 0.01, float), ('noise_std_smplx_betas', 0.1, float),
    ('batch_size', 64, int), ('infill_traj', False, _bool), ('max_infill_ratio', 0.1, float), ('visualize', True, _bool)]
SPECS = {'amass_full': AMASS_FULL, 'prox_egobody': PROX_EGOBODY, 'posenet': POSENET, 'trajnet': TRAJNET}
# prox_egobody's arguments without the directory layout; the save root is the package's choice
TRACK = [(n, 'test_results/results_track' if n == 'save_root' else d, t) for n, d, t in PROX_EGOBODY
         if n not in ('dataset', 'dataset_root', 'init_root', 'recording_name')]
# the package's own arguments (everything above is the scripts')
_SAVE = [('save_interval', 0, int), ('evaluate', False, _bool)]
OWN = {'amass_full': [('eval_noise_root', 'data/eval_noise_smplx', str)] + _SAVE,
       'prox_egobody': [('rohm_root', '', str), ('floor_heights', '', str)] + _SAVE,
       'posenet': _SAVE, 'trajnet': [('evaluate', False, _bool)],
       'track': [('track', '', str), ('tail', 'cover', str), ('max_gap', None, lambda s: None if s in ('', 'None', 'none') else float(s))]
       + _SAVE}
CHOICES = {'noise_schedule': ['linear', 'cosine'], 'task': ['traj', 'pose'], 'mask_scheme': ['lower', 'upper', 'full'],
           'dataset': ['prox', 'egobody'], 'tail': ['cover', 'drop']}
USAGE = 'usage: python -m rohm_amd.drivers amass_full|prox_egobody|posenet|trajnet|track [--config cfg.yaml] [--key value ...]'


def parse_args(which, argv):
    """Namespace of the driver's arguments: defaults, then the config file's values, then the command line's."""
    spec = (TRACK if which == 'track' else SPECS[which]) + OWN[which]
    pre = argparse.ArgumentParser(add_help=False)
    pre.add_argument('--config', default='')
    known, _ = pre.parse_known_args(argv)
    parser = argparse.ArgumentParser(prog=f'python -m rohm_amd.drivers {which}', description='RoHM inference on an AMD GPU')
    parser.add_argument('--config', default='', help='config file path')
    for name, default, typ in spec:
        if name == 'evaluate':          # a bare `--evaluate` switches it on
            parser.add_argument('--evaluate', nargs='?', const=True, default=default, type=typ)
        else:
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
    return parser.parse_args(argv)


def fixseed(seed):
    """utils/fixseed.py."""
    torch.backends.cudnn.benchmark = False
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def _make_body_model(body_model_path, device):
    """The neutral SMPL-X model of `smplx.create(model_path=..., gender='neutral', flat_hand_mean=True, use_pca=False)`: an
    SMPLX_NEUTRAL.npz under the path read natively, or smplx where it is installed."""
    from ..data_loaders.dataloader_video import _body_model
    return _body_model(body_model_path, 'neutral', device)


def _logdir(model_path):
    return '/'.join(model_path.split('/')[0:-1])


def _load_posenet(model, path, strict=True):
    """`model.load_state_dict(torch.load(path), strict)` for the network's own 108 keys.  `smplx_model.*` entries are the body
    model's buffers as the smplx package names them; the body model here is read from --body_model_path (the same file), so
    they are neither loaded nor required."""
    weights = {k: v for k, v in _load(path).items() if not k.startswith('smplx_model.')}
    own = {k for k in model.state_dict() if not k.startswith('smplx_model.')}
    if strict and own != set(weights):
        raise RuntimeError(f'{path}: missing keys {sorted(own - set(weights))[:6]}, unexpected keys {sorted(set(weights) - own)[:6]}')
    model.load_state_dict(weights, strict=False)
    return model.eval()


def _posenet(args, dataset, body, device, path, strict=True):
    from ..model.posenet import PoseNet
    print('[INFO] loaded PoseNet checkpoint path:', path)
    model = PoseNet(dataset=dataset, body_feat_dim=dataset.body_feat_dim, latent_dim=512, ff_size=1024, num_layers=8, num_heads=4,
                    dropout=0.1, activation="gelu", body_model_path=body, device=device, traj_feat_dim=dataset.traj_feat_dim).to(device)
    return _load_posenet(model, path, strict)


def _trajnet(args, dataset, device, path, trajcontrol):
    from ..model.trajnet import TrajNet
    print('[INFO] loaded TrajNet{} checkpoint path:'.format(' TrajControl' if trajcontrol else ''), path)
    model = TrajNet(time_dim=32, mid_dim=512, cond_dim=dataset.traj_feat_dim, traj_feat_dim=dataset.traj_feat_dim,
                    trajcontrol=trajcontrol, device=device, dataset=dataset, repr_abs_only=args.repr_abs_only).to(device)
    model.load_state_dict(_load(path))
    return model.eval()


def _diffusion(args, kind, steps, device):
    from ..diffusion import gaussian_diffusion_posenet, gaussian_diffusion_trajnet
    from ..diffusion.respace import SpacedDiffusionPoseNet, SpacedDiffusionTrajNet
    from ..utils.model_util import create_gaussian_diffusion
    gd, cls = {'posenet': (gaussian_diffusion_posenet, SpacedDiffusionPoseNet),
               'trajnet': (gaussian_diffusion_trajnet, SpacedDiffusionTrajNet)}[kind]
    return create_gaussian_diffusion(args, gd=gd, return_class=cls, num_diffusion_timesteps=steps,
                                     timestep_respacing=args.timestep_respacing_eval, device=device)


def _two_stage(args, pose_dataset, traj_dataset, body, device):
    """test_amass_full.py:130-188 / test_prox_egobody.py:110-168: the three networks and their samplers."""
    print("creating model and diffusion...")
    models = {'posenet': _posenet(args, pose_dataset, body, device, args.model_path_posenet),
              'trajnet': _trajnet(args, traj_dataset, device, args.model_path_trajnet, False),
              'trajnet_control': _trajnet(args, traj_dataset, device, args.model_path_trajnet_control, True)}
    diffusions = {'posenet': _diffusion(args, 'posenet', args.diffusion_steps_posenet, device),
                  'trajnet': _diffusion(args, 'trajnet', args.diffusion_steps_trajnet, device),
                  'trajnet_control': _diffusion(args, 'trajnet', args.diffusion_steps_trajnet, device)}
    return models, diffusions


def _scheduled(pose_dataset, traj_dataset, batch_size, make):
    """The scripts' loop over `len(dataset) // batch_size + 1` steps with both iterators restarted on exhaustion: yields
    (pose batch, traj batch) per step.  `make(dataset)` is a fresh iterator over the dataset's batches."""
    from .results import step_schedule
    src = {'pose': pose_dataset, 'traj': traj_dataset}
    its = {k: make(v) for k, v in src.items()}

    def nxt(which):
        try:
            return next(its[which])
        except StopIteration:
            its[which] = make(src[which])
            return next(its[which])
    for _ in step_schedule(len(pose_dataset), batch_size):
        yield nxt('pose'), nxt('traj')


def _print_lines(lines):
    for ln in lines:
        print(ln)
    return lines


# ---- test_amass_full.py -------------------------------------------------------------------------------------------------------------
def main_amass_full(args):
    from ..data_loaders.dataloader_amass import DataloaderAMASS
    from ..evaluation import amass_lines, amass_metrics
    from ..inference import run_amass_iterations
    from . import results as R
    device = f'cuda:{args.device}'
    print("creating data loader...")
    noise = None
    if args.load_noise:                                                                            # :84-89
        with open(os.path.join(args.eval_noise_root, 'smplx_noise_level_{}.pkl'.format(args.load_noise_level)), 'rb') as f:
            noise = pickle.load(f)
    body = _make_body_model(args.body_model_path, device)
    kw = dict(preprocessed_amass_root=args.dataset_root, split='test', amass_datasets=TEST_DATASETS, body_model_path=body,
              input_noise=args.input_noise, noise_std_smplx_global_rot=args.noise_std_smplx_global_rot,
              noise_std_smplx_body_rot=args.noise_std_smplx_body_rot, noise_std_smplx_trans=args.noise_std_smplx_trans,
              noise_std_smplx_betas=args.noise_std_smplx_betas, load_noise=args.load_noise, loaded_smplx_noise_dict=noise,
              clip_len=args.clip_len, device=device)
    pose_dataset = DataloaderAMASS(task='pose', logdir=_logdir(args.model_path_posenet), **kw)
    traj_dataset = DataloaderAMASS(task='traj', repr_abs_only=args.repr_abs_only, logdir=_logdir(args.model_path_trajnet), **kw)
    models, diffusions = _two_stage(args, pose_dataset, traj_dataset, body, device)
    writer = R.ResultWriter(R.amass_full_pickle_path(args), R.AMASS_PICKLE_KEYS,
                            dict(R.repr_static(), mask_scheme=args.mask_scheme), save_interval=args.save_interval)
    kept = []
    for batch_pose, batch_traj in _scheduled(pose_dataset, traj_dataset, args.batch_size,
                                             lambda ds: ds.batches(args.batch_size, shuffle=False)):
        traj_noisy_full = batch_traj['motion_repr_noisy'][:, :, 0:22].clone()                      # :252
        val_output_pose, _, _ = run_amass_iterations(args, models, diffusions, batch_traj, batch_pose, traj_dataset, pose_dataset,
                                                     body)
        res = R.amass_full_results(val_output_pose, batch_pose, traj_noisy_full, pose_dataset, body, args.input_noise)
        writer.add(res)
        print('current data saved.')
        if args.evaluate:
            kept.append(res)
    path = writer.close()
    print('test finished.')
    lines = []
    if args.evaluate and kept:
        if args.mask_scheme == 'upper':
            print("[rohm_amd.drivers] eval_amass_full.py defines its metrics for mask_scheme 'lower' and 'full' only")
        else:
            cat = lambda k: torch.cat([r[k] for r in kept], dim=0)      # noqa: E731
            m = amass_metrics(cat('rec_ric_data_clean_list'), cat('rec_ric_data_rec_list_from_smpl'), cat('motion_repr_clean_list'),
                              cat('motion_repr_rec_list'), args.mask_scheme, args.traj_mask_ratio if args.infill_traj else 0.0)
            lines = _print_lines(amass_lines(m))
    return {'path': path, 'lines': lines}


# ---- test_prox_egobody.py -----------------------------------------------------------------------------------------------------------
def _floor_heights(args):
    """--floor_heights: a JSON file of floor heights (m) keyed by scene, as DataloaderVideo takes them, or by recording, as
    rohm_amd.evaluation takes them: the recording's entry is filed under its scene."""
    if not args.floor_heights:
        return None
    import json
    with open(args.floor_heights) as f:
        table = {str(k): float(v) for k, v in json.load(f).items()}
    if args.recording_name in table:
        if args.dataset == 'prox':
            scene = args.recording_name.split('_')[0]
        else:
            from ..evaluation import read_egobody_scenes
            scene = read_egobody_scenes(args.dataset_root)[args.recording_name]
        table[scene] = table[args.recording_name]
    return table


def main_prox_egobody(args):
    from ..data_loaders.dataloader_video import DataloaderVideo
    from ..evaluation import scene_metrics
    from ..inference import run_prox_iterations
    from . import results as R
    device = f'cuda:{args.device}'
    print("creating data loader...")
    body = _make_body_model(args.body_model_path, device)
    # EgoBody's ground truth takes the gendered models under the path; PROX needs the neutral one only
    kw = dict(dataset=args.dataset, init_root=args.init_root, base_dir=args.dataset_root,
              body_model_path=body if args.dataset == 'prox' else args.body_model_path,
              recording_name=args.recording_name, use_scene_floor_height=args.use_scene_floor_height, clip_len=args.clip_len,
              overlap_len=args.window_size, device=device, floor_heights=_floor_heights(args), rohm_root=args.rohm_root or None)
    pose_dataset = DataloaderVideo(task='pose', logdir=_logdir(args.model_path_posenet), **kw)
    traj_dataset = DataloaderVideo(task='traj', repr_abs_only=args.repr_abs_only, logdir=_logdir(args.model_path_trajnet), **kw)
    models, diffusions = _two_stage(args, pose_dataset, traj_dataset, body, device)
    static = dict(R.repr_static(), recording_name=pose_dataset.recording_name)
    if args.dataset == 'egobody':
        static['gender_gt'] = pose_dataset.gender_gt
    writer = R.ResultWriter(R.prox_egobody_pickle_path(args, pose_dataset.recording_name), R.SCENE_PICKLE_KEYS, static,
                            last_only=('frame_name_list',), save_interval=args.save_interval)
    report = None
    for batch_pose, batch_traj in _scheduled(pose_dataset, traj_dataset, args.batch_size, lambda ds: ds.batches(args.batch_size)):
        val_output_joint, _, _ = run_prox_iterations(args, models, diffusions, batch_traj, batch_pose, traj_dataset, pose_dataset, body)
        res = R.prox_egobody_results(val_output_joint, batch_pose, pose_dataset, body, args.dataset)
        writer.add(res)
        print('current data saved.')
        if args.evaluate:
            if pose_dataset.scene_floor_height is None:
                raise ValueError('--evaluate needs the floor height: give --floor_heights or --rohm_root')
            ego = args.dataset == 'egobody'
            m = scene_metrics(res['rec_ric_data_rec_list_from_smpl'], res['trans_scene2cano_list'], pose_dataset.scene_floor_height,
                              args.dataset, joints_gt=res['joints_gt_scene_coord_list'] if ego else None,
                              mask_joint_vis=res['mask_joint_vis_list'] if ego else None)
            report = m if report is None else report.merge(m)
    path = writer.close()
    print('test finished.')
    lines = _print_lines(report.lines()) if report is not None else []
    return {'path': path, 'lines': lines, 'report': report}


# ---- a generic track ------------------------------------------------------------------------------------------------------------------
def main_track(args):
    """`main_prox_egobody` on two `DataloaderTrack`s.  The pickle has the scripts' keys plus what `rohm_amd.export --dataset track`
    needs to put the reconstruction back on the source's time stamps: times_dst, src_index, gap (per 30 fps frame), clip_starts,
    times_src, valid, source_frame_names and cam2world."""
    from ..data_loaders.track import DataloaderTrack, read_track
    from ..inference import run_prox_iterations
    from . import results as R
    if args.evaluate:
        raise ValueError('--evaluate is not available for tracks: there is no ground truth, and the scene metrics are defined for '
                         'PROX and EgoBody only')
    if not args.track:
        raise ValueError('give --track file.npz')
    device = f'cuda:{args.device}'
    print("creating data loader...")
    track = read_track(args.track)
    if args.cond_fn_with_grad and not track['has_keypoints']:
        raise ValueError('--cond_fn_with_grad True guides PoseNet with the 2-D keypoints: the track needs keypoints_2d and the '
                         'camera (focal_length and camera_center, or camera_mtx with dist_coeffs); run with --cond_fn_with_grad False')
    body = _make_body_model(args.body_model_path, device)
    kw = dict(body_model_path=body, use_scene_floor_height=args.use_scene_floor_height, clip_len=args.clip_len,
              overlap_len=args.window_size, tail=args.tail, max_gap=args.max_gap, device=device)
    pose_dataset = DataloaderTrack(track, task='pose', logdir=_logdir(args.model_path_posenet), **kw)
    traj_dataset = DataloaderTrack(track, task='traj', repr_abs_only=args.repr_abs_only, logdir=_logdir(args.model_path_trajnet), **kw)
    models, diffusions = _two_stage(args, pose_dataset, traj_dataset, body, device)
    extra = {'times_dst': pose_dataset.times_dst, 'src_index': pose_dataset.src_index, 'gap': pose_dataset.gap,
             'clip_starts': np.asarray(pose_dataset.clip_starts), 'times_src': pose_dataset.times_src, 'valid': pose_dataset.valid,
             'source_frame_names': np.asarray(track['frame_names']), 'cam2world': np.asarray(track['cam2world'])}
    static = dict(R.repr_static(), recording_name=pose_dataset.recording_name, **extra)
    args.dataset = 'track'
    writer = R.ResultWriter(R.prox_egobody_pickle_path(args, pose_dataset.recording_name), R.SCENE_PICKLE_KEYS + list(extra), static,
                            last_only=('frame_name_list',), save_interval=args.save_interval)
    for batch_pose, batch_traj in _scheduled(pose_dataset, traj_dataset, args.batch_size, lambda ds: ds.batches(args.batch_size)):
        val_output_joint, _, _ = run_prox_iterations(args, models, diffusions, batch_traj, batch_pose, traj_dataset, pose_dataset, body)
        writer.add(R.prox_egobody_results(val_output_joint, batch_pose, pose_dataset, body, 'prox'))
        print('current data saved.')
    path = writer.close()
    print('test finished.')
    return {'path': path, 'lines': []}


# ---- test_posenet.py ----------------------------------------------------------------------------------------------------------------
def _amass_dataset(args, body, device, **kw):
    from ..data_loaders.dataloader_amass import DataloaderAMASS
    return DataloaderAMASS(preprocessed_amass_root=args.dataset_root, split='test', amass_datasets=TEST_DATASETS,
                           body_model_path=body, input_noise=args.input_noise,
                           noise_std_smplx_global_rot=args.noise_std_smplx_global_rot,
                           noise_std_smplx_body_rot=args.noise_std_smplx_body_rot, noise_std_smplx_trans=args.noise_std_smplx_trans,
                           noise_std_smplx_betas=args.noise_std_smplx_betas, task=args.task, clip_len=args.clip_len,
                           logdir=_logdir(args.model_path), device=device, **kw)


def _viewer_note(args):
    if args.visualize:
        print('[rohm_amd.drivers] the interactive viewer is not part of the package: pictures come from '
              '`python -m rohm_amd.evaluation --render`')


def main_posenet(args):
    from ..inference import apply_occlusion_mask
    from . import results as R
    device = f'cuda:{args.device}'
    print("creating data loader...")
    body = _make_body_model(args.body_model_path, device)
    dataset = _amass_dataset(args, body, device, repr_abs_only=False)
    print("creating model and diffusion...")
    model = _posenet(args, dataset, body, device, args.model_path, strict=False)                    # :93
    diffusion = _diffusion(args, 'posenet', args.diffusion_steps, device)
    _viewer_note(args)
    writer = R.ResultWriter(R.posenet_pickle_path(args), R.POSENET_PICKLE_KEYS, R.repr_static(), save_interval=args.save_interval)
    reports, last = [], None
    for batch in dataset.batches(args.batch_size, shuffle=False):
        cond = (batch['motion_repr_noisy'] if args.input_noise else batch['motion_repr_clean']).clone()      # :136-139
        bs, clip_len = batch['motion_repr_clean'].shape[:2]
        start = end = None
        if args.mask_scheme == 'full':                                                              # :165-169
            start = torch.FloatTensor(bs).uniform_(0, clip_len - 1).long()
            end = torch.clamp(start + 30, max=clip_len)
        apply_occlusion_mask(cond, args.mask_scheme, dataset.traj_feat_dim, start, end)
        batch['motion_repr_clean'] = batch['motion_repr_clean'].permute(0, 2, 1).unsqueeze(-2)      # :175-176
        batch['cond'] = cond.permute(0, 2, 1).unsqueeze(-2)
        losses, val_output = diffusion.eval_losses(model=model, batch=batch, shape=list(batch['motion_repr_clean'].shape),
                                                   progress=False, clip_denoised=False,
                                                   timestep_respacing=args.timestep_respacing_eval,
                                                   cond_fn_with_grad=args.cond_fn_with_grad, smplx_model=body)
        if args.evaluate:
            reports.append({k: v.detach() for k, v in losses.items()})
        if args.save_results:
            if last is not None:
                R.threshold_contact_labels(last)                                                    # :260-265, see results.py
            last = writer.add(R.posenet_results(val_output, batch, dataset, body, args.input_noise))
            print('current data saved.')
    path = writer.close() if args.save_results else None
    lines = []
    if reports:
        lines = _print_lines(['[EVAL] {}: {:0.10f}'.format(k, float(torch.stack([r[k] for r in reports]).mean())) for k in reports[0]])
    return {'path': path, 'lines': lines}


# ---- test_trajnet.py ----------------------------------------------------------------------------------------------------------------
def traj_infill_window(batch_size, clip_len, max_infill_ratio, traj_feat_dim, device):
    """test_trajnet.py:139-148: a random window per clip hidden -> mask [bs, T, traj_feat_dim], 1 = visible."""
    start = torch.FloatTensor(batch_size).uniform_(0, clip_len - 1).long()
    mask_len = (clip_len * torch.FloatTensor(batch_size).uniform_(0, 1) * max_infill_ratio).long()
    end = torch.clamp(start + mask_len, max=clip_len)
    frames = torch.arange(clip_len)[None]
    hide = (frames >= start[:, None]) & (frames < end[:, None])
    return (~hide).float().to(device).unsqueeze(-1).repeat(1, 1, traj_feat_dim)


def main_trajnet(args):
    from . import results as R
    device = f'cuda:{args.device}'
    print("creating data loader...")
    body = _make_body_model(args.body_model_path, device)
    dataset = _amass_dataset(args, body, device, repr_abs_only=args.repr_abs_only)
    print("creating model and diffusion...")
    model = _trajnet(args, dataset, device, args.model_path, args.trajcontrol)
    diffusion = _diffusion(args, 'trajnet', args.diffusion_steps, device)
    _viewer_note(args)
    tfd = dataset.traj_feat_dim
    report = None
    for batch in dataset.batches(args.batch_size, shuffle=False):
        bs, clip_len = batch['cond'].shape[:2]
        if args.infill_traj:                                                                        # :139-149
            mask_traj = traj_infill_window(bs, clip_len, args.max_infill_ratio, tfd, device)
            batch['cond'][:, :, 0:tfd] = batch['cond'][:, :, 0:tfd] * mask_traj
        shape = list(batch['motion_repr_clean'][:, :, 0:tfd].shape)
        _, val_output = diffusion.eval_losses(model=model, batch=batch, shape=shape, progress=False, clip_denoised=False,
                                              timestep_respacing=args.timestep_respacing_eval, cond_fn_with_grad=False,
                                              compute_loss=False, smplx_model=body)      # the script never reads the loss report
        res = R.trajnet_results(val_output, batch, dataset, body, args.repr_abs_only)
        m = R.traj_report([res['rec_ric_data_' + k] for k in ('clean', 'noisy', 'rec_from_abs_traj', 'rec_from_rel_traj',
                                                              'rec_from_smpl')],
                          res['motion_repr_clean'], res['motion_repr_clean_root_rec'])
        report = m if report is None else report.merge(m)
    lines = _print_lines(report.lines()) if report is not None else []
    return {'path': None, 'lines': lines, 'report': report}


MAINS = {'amass_full': main_amass_full, 'prox_egobody': main_prox_egobody, 'posenet': main_posenet, 'trajnet': main_trajnet,
         'track': main_track}


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv or argv[0] not in MAINS:
        raise SystemExit(USAGE)
    args = parse_args(argv[0], argv[1:])
    fixseed(args.seed)
    return MAINS[argv[0]](args)


if __name__ == '__main__':
    main()
