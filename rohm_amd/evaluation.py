"""Evaluation metrics of the drivers on the device: AMASS (eval_amass_full.py:67-147) and
PROX / EgoBody (eval_prox_egobody.py:172-270), plus a headless evaluator of the drivers' pickles
(`python -m rohm_amd.evaluation`), which with `--render` also writes the scripts' pictures (rohm_amd.render).

`amass_metrics` takes what test_amass_full.py:387-429 produces (recovered joints of the clean clips and of the
reconstruction, the de-normalised representations) as device tensors and returns the quantities the evaluation
script prints, in its units.  One kernel launch (`rohm_amass_metrics`), one small D2H copy of the per-clip sums.

`scene_metrics` does the same for the PROX / EgoBody driver (`rohm_scene_metrics`): back to scene coordinates,
skating, acceleration, (EgoBody) MPJPE split by visibility, ground penetration, as per-clip sums in a `SceneMetrics`.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr

LOWER_JOINTS = (1, 2, 4, 5, 7, 8, 10, 11)          # eval_amass_full.py:76


def amass_metrics(joints_clean, joints_rec, repr_clean, repr_rec, mask_scheme='lower', traj_mask_ratio=0.0):
    """joints_*: [n_seq, clip_len, 22, 3]; repr_*: [n_seq, clip_len, 294] de-normalised.  Returns a dict with the
    script's names and units: mpjpe_global[_vis|_occ] (mm), contact_lbl_acc, skating_gt_ratio, skating_rec_ratio,
    accel_error (m/s^2), ground_pene_freq (%), ground_pene_dist (mm)."""
    for t in (joints_clean, joints_rec, repr_clean, repr_rec):
        _lib.require_hip(t)
    jc, jr = joints_clean.float().contiguous(), joints_rec.float().contiguous()
    if jc.shape != jr.shape or jc.dim() != 4 or jc.shape[2:] != (22, 3):
        raise ValueError(f'joints must both be [n_seq, clip_len, 22, 3], got {tuple(jc.shape)} / {tuple(jr.shape)}')
    n, T = jc.shape[:2]
    rc, rr = repr_clean.float().contiguous(), repr_rec.float().contiguous()
    if rc.shape != (n, T, 294) or rr.shape != (n, T, 294):
        raise ValueError('representations must be [n_seq, clip_len, 294]')
    mask, start, end = 0, 0, 0
    if mask_scheme == 'lower':
        for j in LOWER_JOINTS:
            mask |= 1 << j
    elif mask_scheme == 'full':
        start = 65
        end = start + int(traj_mask_ratio * 145)
    else:
        raise ValueError(f'unknown mask_scheme {mask_scheme!r}')
    out = torch.empty(n, 10, device=jc.device, dtype=torch.float64)
    check(lib().rohm_amass_metrics(ptr(jc), ptr(jr), rc.data_ptr() + 290 * 4, 294, rr.data_ptr() + 290 * 4, 294, mask,
                                   start, end, n, T, ptr(out), stream_ptr(jc.device)), 'rohm_amass_metrics')
    s = out.sum(dim=0).cpu().tolist()
    tot = n * T * 22
    n_occ = s[2]
    res = {'mpjpe_global': s[0] / tot * 1000.0,
           'mpjpe_global_vis': (s[0] - s[1]) / max(tot - n_occ, 1.0) * 1000.0,
           'mpjpe_global_occ': s[1] / max(n_occ, 1.0) * 1000.0,
           'contact_lbl_acc': s[3] / (n * T * 4),
           'skating_gt_ratio': s[4] / (n * (T - 1)),
           'skating_rec_ratio': s[5] / (n * (T - 1)),
           'accel_error': s[6] / (n * (T - 2) * 22),
           'ground_pene_freq': s[7] / (n * T * 2) * 100.0,
           'ground_pene_dist': s[8] / (n * T * 2) * 1000.0}
    return res


# ---- PROX / EgoBody (eval_prox_egobody.py:172-270, final block :453-490) -------------------------------------------

SCENE_UP_AXIS = {'prox': 2, 'egobody': 1}          # :190-199: PROX scene coordinates are z-up, EgoBody's y-up
_N_SCENE = 11                                       # rohm_scene_metrics output layout, include/rohm_hip.h
SCENE_MAX_T = 800


class SceneMetrics:
    """Per-clip sums of `rohm_scene_metrics` (float64, host, [n_clip, 11], layout in include/rohm_hip.h) for clips of
    one length.  The script's per-recording and 'all' numbers are means over concatenated clips, i.e. exactly sums of
    these sums divided by counts: `merge` concatenates, `summary` divides."""

    def __init__(self, dataset, clip_len, sums):
        if dataset not in SCENE_UP_AXIS:
            raise ValueError(f"dataset must be 'prox' or 'egobody', got {dataset!r}")
        self.dataset, self.clip_len = dataset, int(clip_len)
        self.sums = np.asarray(sums, dtype=np.float64).reshape(-1, _N_SCENE)

    @property
    def n_clips(self):
        return len(self.sums)

    def merge(self, *others):
        for o in others:
            if o.dataset != self.dataset or o.clip_len != self.clip_len:
                raise ValueError(f'cannot merge {o.dataset}/T={o.clip_len} into {self.dataset}/T={self.clip_len}')
        return SceneMetrics(self.dataset, self.clip_len, np.concatenate([self.sums] + [o.sums for o in others], axis=0))

    def summary(self):
        """The script's names and units (:477-490): skating (ratio), acc (PROX) or acc_error (EgoBody) in m/s^2,
        ground_pene_freq (%), ground_pene_dist (mm, positive); EgoBody also gmpjpe / mpjpe / mpjpe_vis / mpjpe_occ
        (mm; vis / occ are sum / mask sum, nan for an empty mask as numpy's 0 / 0)."""
        n, T = self.n_clips, self.clip_len
        s = self.sums.sum(axis=0)
        res = {'skating': s[0] / (n * (T - 1))}
        if self.dataset == 'prox':
            res['acc'] = s[1] / (n * (T - 2) * 22)
        else:
            res['acc_error'] = s[2] / (n * (T - 2) * 22)
        res['ground_pene_freq'] = s[3] / (n * T * 2) * 100.0
        res['ground_pene_dist'] = -s[4] / (n * T * 2) * 1000.0
        if self.dataset == 'egobody':
            res['gmpjpe'] = s[5] / (n * T * 22) * 1000.0
            res['mpjpe'] = s[6] / (n * T * 22) * 1000.0
            with np.errstate(divide='ignore', invalid='ignore'):
                res['mpjpe_vis'] = float(np.float64(s[7]) / np.float64(s[8]) * 1000.0)
                res['mpjpe_occ'] = float(np.float64(s[9]) / np.float64(s[10]) * 1000.0)
        return {k: float(v) for k, v in res.items()}

    def lines(self):
        """The lines the script's final block prints (:477-490)."""
        m = self.summary()
        out = ['\n --------------- evaluation metrics -------------', 'skating score: {:0.3f}'.format(m['skating'])]
        if self.dataset == 'prox':
            out.append('||acc|| (m/s^2): {:0.2f}'.format(m['acc']))
        else:
            out.append('acc errors (m/s^2): {:0.2f}'.format(m['acc_error']))
        out.append('ground_pene_freq score (%): {:0.2f}'.format(m['ground_pene_freq']))
        out.append('ground_pene_dist score (mm): {:0.2f}'.format(m['ground_pene_dist']))
        if self.dataset == 'egobody':
            out.append('-------------- gmpjpe/mpjpe/mpjpe-vis/mpjpe-occ (mm) --------------')
            out.append('{:0.2f} / {:0.2f} / {:0.2f} / {:0.2f}'.format(m['gmpjpe'], m['mpjpe'], m['mpjpe_vis'], m['mpjpe_occ']))
        return out


def _ground_vector(ground_height, B, dev):
    if isinstance(ground_height, torch.Tensor):
        _lib.require_hip(ground_height)
        g = ground_height.detach().to(torch.float32).reshape(-1)
    else:
        # rounded to float32 like numpy's weak Python scalar against a float32 array (NEP 50)
        g = torch.from_numpy(np.asarray(ground_height, dtype=np.float64).astype(np.float32).reshape(-1)).to(dev)
    if g.numel() == 1:
        g = g.expand(B)
    if g.numel() != B:
        raise ValueError(f'ground_height: need one value or one per clip ({B}), got {g.numel()}')
    return g.contiguous()


def scene_metrics(joints_rec, trans_scene2cano, ground_height, dataset, joints_gt=None, mask_joint_vis=None,
                  return_joints_scene=False):
    """eval_prox_egobody.py:172-270 on the device.  joints_rec [n_clip, T, 22, 3] in canonical coordinates (the
    driver's `rec_ric_data_rec_list_from_smpl`), trans_scene2cano [n_clip, 4, 4], ground_height one float or one per
    clip (metres, scene coordinates), dataset 'prox' | 'egobody'.  EgoBody also needs joints_gt [n_clip, T_gt >= T,
    22, 3] in scene coordinates and mask_joint_vis [n_clip, T, 22].  One launch, one small D2H copy.  Returns a
    `SceneMetrics` (and the back-transformed joints [n_clip, T, 22, 3] if `return_joints_scene`)."""
    if dataset not in SCENE_UP_AXIS:
        raise ValueError(f"dataset must be 'prox' or 'egobody', got {dataset!r}")
    for t in (joints_rec, trans_scene2cano, joints_gt, mask_joint_vis):
        if t is not None and not isinstance(t, torch.Tensor):
            raise TypeError('scene_metrics takes torch tensors on a HIP device')
        _lib.require_hip(t)
    jr = joints_rec.detach().float().contiguous()
    if jr.dim() != 4 or jr.shape[2:] != (22, 3):
        raise ValueError(f'joints_rec must be [n_clip, T, 22, 3], got {tuple(jr.shape)}')
    B, T = jr.shape[:2]
    if not 3 <= T <= SCENE_MAX_T:
        raise ValueError(f'clip length must be in [3, {SCENE_MAX_T}], got {T}')
    m = trans_scene2cano.detach().float().contiguous()
    if m.shape != (B, 4, 4):
        raise ValueError(f'trans_scene2cano must be [{B}, 4, 4], got {tuple(m.shape)}')
    if dataset == 'egobody' and (joints_gt is None or mask_joint_vis is None):
        raise ValueError('egobody needs joints_gt and mask_joint_vis')
    if mask_joint_vis is not None and joints_gt is None:
        raise ValueError('mask_joint_vis is only used with joints_gt')
    jg = mk = None
    T_gt = 0
    if joints_gt is not None:
        jg = joints_gt.detach().float().contiguous()
        if jg.dim() != 4 or jg.shape[0] != B or jg.shape[1] < T or jg.shape[2:] != (22, 3):
            raise ValueError(f'joints_gt must be [{B}, T_gt >= {T}, 22, 3], got {tuple(jg.shape)}')
        T_gt = jg.shape[1]
    if mask_joint_vis is not None:
        mk = mask_joint_vis.detach().float().contiguous()
        if mk.shape != (B, T, 22):
            raise ValueError(f'mask_joint_vis must be [{B}, {T}, 22] (the driver slices it to T frames), '
                             f'got {tuple(mk.shape)}')
    dev = jr.device
    g = _ground_vector(ground_height, B, dev)
    js = torch.empty_like(jr) if return_joints_scene else None
    out = torch.empty(B, _N_SCENE, device=dev, dtype=torch.float64)
    check(lib().rohm_scene_metrics(ptr(jr), ptr(m), ptr(g), SCENE_UP_AXIS[dataset], ptr(jg), T_gt, ptr(mk), ptr(js), B, T,
                                   ptr(out), stream_ptr(dev)), 'rohm_scene_metrics')
    res = SceneMetrics(dataset, T, out.cpu().numpy())
    return (res, js) if return_joints_scene else res


def scene_metrics_from_output(val_output_joint, pose_dataset, smplx_model, transf_matrix, ground_height, dataset,
                              joints_gt=None, mask_joint_vis=None):
    """Score what `run_prox_iterations` returns without leaving the device: the driver's joint recovery
    (test_prox_egobody.py:326-357: de-normalise, recover_from_repr_smpl 'smplx_params') followed by `scene_metrics`.
    val_output_joint [n_clip, 294, 1, T] normalised; transf_matrix = the batch's 'transf_matrix' (scene -> canonical).
    mask_joint_vis must be sliced as the driver slices it, `mask_joint_vis[:, 0:-2]` (test_prox_egobody.py:307), i.e. the
    T frames of the output."""
    from .data_loaders.motion_representation import joints_from_repr
    joints = joints_from_repr(val_output_joint, 'smplx_params', smplx_model, stats=pose_dataset, layout='bc1t')
    return scene_metrics(joints, transf_matrix, ground_height, dataset, joints_gt=joints_gt, mask_joint_vis=mask_joint_vis)


# ---- headless evaluator: python -m rohm_amd.evaluation ---------------------------------------------------------------

def read_floor_heights(rohm_root, dataset):
    """The `prox_floor_height` / `egobody_floor_height` dict literal of a RoHM checkout's utils/other_utils.py, read
    with `ast` (the module itself imports cv2)."""
    import ast
    name = f'{dataset}_floor_height'
    path = os.path.join(rohm_root, 'utils', 'other_utils.py')
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == name for t in node.targets):
            return {str(k): float(v) for k, v in ast.literal_eval(node.value).items()}
    raise KeyError(f'{name} not found in {path}')


def read_egobody_scenes(dataset_root):
    """recording_name -> scene_name from <dataset_root>/egobody_rohm_info.csv (eval_prox_egobody.py:75-91)."""
    import csv
    with open(os.path.join(dataset_root, 'egobody_rohm_info.csv'), newline='') as f:
        return {row['recording_name']: row['scene_name'] for row in csv.DictReader(f)}


def recording_floor_heights(dataset, recordings, floor_heights=None, rohm_root=None, dataset_root=None):
    """recording -> ground height: from a JSON file (recording -> metres), or from a RoHM checkout's tables keyed by
    scene (PROX: the recording name's first field, :121; EgoBody: the scene column of egobody_rohm_info.csv)."""
    if floor_heights:
        with open(floor_heights) as f:
            table = {str(k): float(v) for k, v in json.load(f).items()}
        missing = [r for r in recordings if r not in table]
        if missing:
            raise KeyError(f'{floor_heights} has no floor height for {missing}')
        return {r: table[r] for r in recordings}
    if not rohm_root:
        raise ValueError('need --floor_heights or --rohm_root')
    table = read_floor_heights(rohm_root, dataset)
    if dataset == 'prox':
        scenes = {r: r.split('_')[0] for r in recordings}
    else:
        if not dataset_root:
            raise ValueError('egobody with --rohm_root needs --dataset_root (for egobody_rohm_info.csv)')
        info = read_egobody_scenes(dataset_root)
        scenes = {r: info[r] for r in recordings}
    return {r: table[s] for r, s in scenes.items()}


AMASS_KEYS = ('rec_ric_data_clean_list', 'rec_ric_data_rec_list_from_smpl', 'motion_repr_clean_list',
              'motion_repr_rec_list')      # eval_amass_full.py:53-66 (what the metrics read)


def amass_lines(m):
    """eval_amass_full.py:73-147's printed lines from `amass_metrics`' dict (both mask schemes print the same ones)."""
    return ['mpjpe_global (mm): {:0.1f}'.format(m['mpjpe_global']),
            'mpjpe_global_vis / occ (mm): {:0.1f} / {:0.1f}'.format(m['mpjpe_global_vis'], m['mpjpe_global_occ']),
            'contact_lbl_acc: {:0.2f}'.format(m['contact_lbl_acc']),
            'skating_gt_ratio: {:0.3f}'.format(m['skating_gt_ratio']),
            'skating_rec_ratio: {:0.3f}'.format(m['skating_rec_ratio']),
            'accel_error (m/s^2): {:0.1f}'.format(m['accel_error']),
            'ground_pene_freq score (%): {:0.2f}'.format(m['ground_pene_freq']),
            'ground_pene_dist score (mm): {:0.2f}'.format(m['ground_pene_dist'])]


def _load(path):
    import pickle
    with open(path, 'rb') as f:
        return pickle.load(f)


def evaluate_amass(saved_data_path, mask_scheme='lower', traj_mask_ratio=0.0, device='cuda:0'):
    d = _load(saved_data_path)
    t = lambda k: torch.as_tensor(np.asarray(d[k], dtype=np.float32)).to(device)
    return amass_metrics(t('rec_ric_data_clean_list'), t('rec_ric_data_rec_list_from_smpl'), t('motion_repr_clean_list'),
                         t('motion_repr_rec_list'), mask_scheme, traj_mask_ratio)


def evaluate_scene(dataset, saved_data_dir, recordings, heights, device='cuda:0'):
    """recording -> SceneMetrics for the driver's pickles <saved_data_dir>/<recording>.pkl (test_prox_egobody.py:361-380)."""
    out = {}
    for rec in recordings:
        d = _load(os.path.join(saved_data_dir, rec + '.pkl'))
        t = lambda k: torch.as_tensor(np.asarray(d[k], dtype=np.float32)).to(device)
        gt = t('joints_gt_scene_coord_list') if dataset == 'egobody' else None
        mask = t('mask_joint_vis_list') if dataset == 'egobody' else None
        out[rec] = scene_metrics(t('rec_ric_data_rec_list_from_smpl'), t('trans_scene2cano_list'), heights[rec], dataset,
                                 joints_gt=gt, mask_joint_vis=mask)
    return out


def _render_body_model(path, dev):
    from .body_model import SMPLXLayer
    from .occlusion import _body_model_file
    return SMPLXLayer.from_npz(_body_model_file(path)).to(dev)


def _load_frames(frames_dir, recording, n, size):
    """`n` already-undistorted colour frames of a recording as uint8 [n, H, W, 3] (and their base names), or None: PIL is
    needed to decode them, and PROX's own frames would first have to be undistorted and flipped (cv2), which is not done here."""
    d = os.path.join(frames_dir, recording)
    if not os.path.isdir(d):
        d = frames_dir
    try:
        from PIL import Image
    except ImportError:
        print(f'[rohm_amd.evaluation] PIL is not installed: rendering {recording} over black', file=sys.stderr)
        return None, None
    names = sorted(f for f in os.listdir(d) if f.lower().endswith(('.png', '.jpg', '.jpeg')))[:n]
    if len(names) < n:
        print(f'[rohm_amd.evaluation] {d} has {len(names)} frames, {n} needed: rendering over black', file=sys.stderr)
        return None, None
    imgs = []
    for f in names:
        with Image.open(os.path.join(d, f)) as im:
            imgs.append(np.asarray(im.convert('RGB').resize(size)) if im.size != tuple(size) else np.asarray(im.convert('RGB')))
    return np.stack(imgs), [os.path.splitext(f)[0] for f in names]


def render_scene_recordings(dataset_root, saved_data_dir, recordings, body_model, out_dir, interval=1, size=(1920, 1080),
                            frames_dir=None, device='cuda:0'):
    """eval_prox_egobody.py:373-451 for PROX: <out_dir>/mesh_skel/<frame>.png (predicted body, skeleton and contacts over
    the background) and <out_dir>/input/<frame>.png (the input body over it), one clip at a time.  Reads
    cam2world/<scene>.json and calibration/Color.json under `dataset_root`, as the script does."""
    from . import render as R
    from .render import _clip_verts
    with open(os.path.join(dataset_root, 'calibration', 'Color.json')) as f:
        color_cam = json.load(f)
    for sub in ('mesh_skel', 'input'):
        os.makedirs(os.path.join(out_dir, sub), exist_ok=True)
    W, H = int(size[0]), int(size[1])
    fxy = (color_cam['f'][0] * W / 1920.0, color_cam['f'][1] * H / 1080.0)
    cxy = (color_cam['c'][0] * W / 1920.0, color_cam['c'][1] * H / 1080.0)
    for rec in recordings:
        with open(os.path.join(dataset_root, 'cam2world', rec.split('_')[0] + '.json')) as f:
            cam2world = np.array(json.load(f), dtype=np.float64)
        d = _load(os.path.join(saved_data_dir, rec + '.pkl'))
        joints = np.asarray(d['rec_ric_data_rec_list_from_smpl'], dtype=np.float32)
        n_seq, T = joints.shape[:2]
        contact = np.asarray(d['motion_repr_rec_list'])[:, :, -4:] > 0.5
        frames, names = _load_frames(frames_dir, rec, n_seq * T, (W, H)) if frames_dir else (None, None)
        for bs in range(0, n_seq, int(interval)):
            v_rec = _clip_verts(d, 'motion_repr_rec_list', bs, body_model, device)[None]
            v_in = _clip_verts(d, 'motion_repr_noisy_list', bs, body_model, device)[None]
            bg = None if frames is None else torch.from_numpy(frames[bs * T:(bs + 1) * T]).to(device)[None]
            got = R.render_scene_clips(v_rec, v_in, torch.from_numpy(joints[bs:bs + 1]).to(device), body_model.faces, cam2world, fxy,
                                       cxy, mask_joint_vis=np.asarray(d['mask_joint_vis_list'])[bs:bs + 1, :T],
                                       contact_lbl=contact[bs:bs + 1], trans_scene2cano=np.asarray(d['trans_scene2cano_list'])[bs:bs + 1],
                                       size=(W, H), background=bg)
            for sub, img in zip(('mesh_skel', 'input'), got):
                host = img[0].cpu().numpy()
                for t in range(T):
                    k = bs * T + t
                    name = names[k] if names else '{}_frame_{:05d}'.format(rec, k)
                    R.write_png(os.path.join(out_dir, sub, name + '.png'), host[t])


def main(argv=None):
    """Headless counterpart of eval_amass_full.py / eval_prox_egobody.py: the metrics, and with --render the pictures, with
    no visualiser, pyrender, cv2, smplx or pandas.  Prints the scripts' final lines; --json also writes the numbers."""
    import argparse
    p = argparse.ArgumentParser(prog='python -m rohm_amd.evaluation', description=main.__doc__)
    p.add_argument('--dataset', required=True, choices=['amass', 'prox', 'egobody'])
    p.add_argument('--saved_data_path', help='amass: the driver pickle')
    p.add_argument('--mask_scheme', default='lower', choices=['lower', 'full'])
    p.add_argument('--traj_mask_ratio', default=0.0, type=float)
    p.add_argument('--saved_data_dir', help='prox / egobody: directory of <recording>.pkl')
    p.add_argument('--recordings', nargs='+', help='default: every *.pkl in --saved_data_dir, sorted')
    p.add_argument('--floor_heights', help='JSON file: recording -> floor height (m)')
    p.add_argument('--rohm_root', help='RoHM checkout: floor heights from utils/other_utils.py')
    p.add_argument('--dataset_root', help='egobody with --rohm_root: directory of egobody_rohm_info.csv')
    p.add_argument('--device', default=0, type=int)
    p.add_argument('--json', help='also write the numbers here')
    truth = lambda x: x.lower() in ['true', '1']
    p.add_argument('--render', nargs='?', const=True, default=False, type=truth,
                   help='also write pictures (PNG): amass pred|input|gt/seq_%%03d/frame_%%03d.png, prox mesh_skel|input/<frame>.png')
    p.add_argument('--render_interval', default=100, type=int, help='render every N clips')
    p.add_argument('--render_save_path', default='render_imgs/render_amass/mask_lower_noise_3', type=str)
    p.add_argument('--body_model_path', type=str, default='data/body_models/smplx_model', help='--render: path to the SMPL-X model')
    p.add_argument('--render_size', nargs=2, type=int, default=[1920, 1080], metavar=('W', 'H'))
    p.add_argument('--vert_segmentation', help="--render, amass 'lower': smplx_vert_segmentation.json (lower body at alpha 0.1)")
    p.add_argument('--frames_dir', help='--render, prox: already-undistorted colour frames (<dir>/<recording>/*); needs PIL')
    a = p.parse_args(argv)
    dev = f'cuda:{a.device}'
    if a.dataset == 'amass':
        if not a.saved_data_path:
            p.error('--dataset amass needs --saved_data_path')
        m = evaluate_amass(a.saved_data_path, a.mask_scheme, a.traj_mask_ratio, dev)
        lines, numbers = amass_lines(m), {'dataset': 'amass', 'all': m}
        if a.render:
            from .render import render_amass
            render_amass(_load(a.saved_data_path), _render_body_model(a.body_model_path, dev), a.mask_scheme, a.traj_mask_ratio,
                         a.render_save_path, a.render_interval, tuple(a.render_size), a.vert_segmentation, device=dev)
    else:
        if not a.saved_data_dir:
            p.error(f'--dataset {a.dataset} needs --saved_data_dir')
        recs = a.recordings or sorted(f[:-4] for f in os.listdir(a.saved_data_dir) if f.endswith('.pkl'))
        if not recs:
            p.error(f'no *.pkl in {a.saved_data_dir}')
        heights = recording_floor_heights(a.dataset, recs, a.floor_heights, a.rohm_root, a.dataset_root)
        per = evaluate_scene(a.dataset, a.saved_data_dir, recs, heights, dev)
        total = per[recs[0]].merge(*[per[r] for r in recs[1:]])
        lines = total.lines()
        numbers = {'dataset': a.dataset, 'all': total.summary(), 'recordings': {r: per[r].summary() for r in recs},
                   'floor_heights': heights}
        if a.render:
            if a.dataset != 'prox':
                p.error("--render covers amass and prox; EgoBody's per-view calibration chain is not read here "
                        '(rohm_amd.render.render_scene_clips is the entry point)')
            if not a.dataset_root:
                p.error('--render with --dataset prox needs --dataset_root (cam2world/, calibration/Color.json)')
            render_scene_recordings(a.dataset_root, a.saved_data_dir, recs, _render_body_model(a.body_model_path, dev),
                                    a.render_save_path, a.render_interval, tuple(a.render_size), a.frames_dir, dev)
    for ln in lines:
        print(ln)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(numbers, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
