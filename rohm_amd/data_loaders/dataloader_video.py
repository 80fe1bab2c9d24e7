"""Native test-time loader of PROX / EgoBody recordings: the reference's `data_loaders/dataloader_video.py` with its
per-frame and per-clip work on the device.

The host part only reads files (standard library + numpy): the per-frame fitting pickles, the OpenPose json files, the
joint-occlusion mask, the calibration json files, the AMASS statistics and, for EgoBody, the two csv files and the
ground-truth fittings.  Everything else is four launches per recording: `frames.frames_to_world` (once more with the
gendered model for EgoBody's ground truth), `clips.build_clips`, `clips.undistort_keypoints` (PROX) and
`clips.visibility_masks`.

`__len__` / `__getitem__` return the reference's items as host numpy (same keys, shapes and dtypes), made from one
device -> host copy at construction, so the object works in a `torch.utils.data.DataLoader` with workers without
touching the GPU there.  `batches(batch_size)` yields the collated dicts as device tensors, with the keys the driver
holds after its `.to(dev)` (test_prox_egobody.py:196-210), ready for `inference.run_prox_iterations`.

One difference: `keypoints_2d` is float32 on the device (the reference holds float64 for PROX; its guidance casts to
float32 anyway).  `__getitem__` keeps the reference's dtype.

The scene floor heights are tables inside the reference's utils/other_utils.py; pass `floor_heights` (a dict or a JSON
file: scene name -> metres) or `rohm_root` (a RoHM checkout, read with `evaluation.read_floor_heights`).  Without
either, `scene_floor_height` is None and `use_scene_floor_height=True` raises."""
from __future__ import annotations

import csv
import json
import os
import pickle

import numpy as np
import torch
from torch.utils import data

from .. import _lib
from . import clips, frames

REPR_DIM_DICT = {'root_rot_angle': 1, 'root_rot_angle_vel': 1, 'root_l_pos': 2, 'root_l_vel': 2, 'root_height': 1,
                 'smplx_rot_6d': 6, 'smplx_rot_vel': 3, 'smplx_trans': 3, 'smplx_trans_vel': 3, 'local_positions': 66,
                 'local_vel': 66, 'smplx_body_pose_6d': 126, 'smplx_betas': 10, 'foot_contact': 4}
REPR_LIST = list(REPR_DIM_DICT)
ABS_TRAJ_CH = (0, 2, 3, 6, 7, 8, 9, 10, 11, 12, 16, 17, 18)             # the repr_abs_only trajectory channels (:492-494)
# OpenPose BODY_25 joint feeding every SMPL joint (:50)
OPENPOSE_TO_SMPL = [8, 12, 9, 8, 13, 10, 8, 14, 11, 1, 20, 23, 1, 5, 2, 0, 5, 2, 6, 3, 7, 4, 7, 4]
PARAM_KEYS = ('transl', 'global_orient', 'betas', 'body_pose')
EGOBODY_SUB_KINECT = {'sub_1': 11, 'sub_2': 13, 'sub_3': 14, 'sub_4': 15}


# ---- host readers ----------------------------------------------------------------------------------------------------------
def read_fitting(path):
    """One `000.pkl` -> dict of float32 rows (transl 3, global_orient 3, betas 10, body_pose 63)."""
    with open(path, 'rb') as f:
        d = pickle.load(f, encoding='latin1')
    row = {k: np.asarray(d[k], dtype=np.float32).reshape(-1) for k in PARAM_KEYS}
    row['betas'] = row['betas'][:10]
    return row


def read_fittings(results_dir, frame_names):
    rows = [read_fitting(os.path.join(results_dir, n, '000.pkl')) for n in frame_names]
    return {k: np.stack([r[k] for r in rows]) for k in PARAM_KEYS}


def read_keypoints(path, joints_num=22, person=0):
    """One OpenPose json -> [joints_num, 3] in SMPL topology: float32, or float64 zeros when nobody was detected."""
    with open(path) as f:
        people = json.load(f)['people']
    if len(people) == 0:
        return np.zeros((joints_num, 3))
    kp = np.array(people[person]['pose_keypoints_2d'], dtype=np.float32).reshape([-1, 3])
    return kp[OPENPOSE_TO_SMPL[0:joints_num]]


def read_json(path):
    with open(path) as f:
        return json.load(f)


def read_stats(logdir):
    """AMASS_mean.pkl / AMASS_std.pkl -> (Mean_dict, Std_dict, Mean [294], Std [294])."""
    with open(os.path.join(logdir, 'AMASS_mean.pkl'), 'rb') as f:
        mean_dict = pickle.load(f, encoding='latin1')
    with open(os.path.join(logdir, 'AMASS_std.pkl'), 'rb') as f:
        std_dict = pickle.load(f, encoding='latin1')
    mean = np.concatenate([mean_dict[k] for k in mean_dict.keys()], axis=-1)
    std = np.concatenate([std_dict[k] for k in std_dict.keys()], axis=-1)
    return mean_dict, std_dict, mean, std


def read_cam2world(dataset, base_dir, recording_name, info=None, return_master=False):
    """The camera -> world transform [4, 4] the loaders apply to a recording's fits: PROX's cam2world/<scene>.json
    (dataloader_video.py:100), EgoBody's calibration chain kinect12_to_world . kinect_<sub>to12_color for a sub view
    (:238-250).  `info`: EgoBody's `read_egobody_info` row when the caller has it already; `return_master` also returns
    EgoBody's master -> world transform."""
    if dataset == 'prox':
        scene_name = recording_name.split('_')[0]
        return np.array(read_json(os.path.join(base_dir, 'cam2world', scene_name + '.json')))
    if dataset != 'egobody':
        raise ValueError(f'dataset {dataset!r} not defined')
    if info is None:
        info = read_egobody_info(base_dir, recording_name)
    view = info['view']
    cal = os.path.join(base_dir, 'calibrations', recording_name, 'cal_trans')
    master2world = np.asarray(read_json(os.path.join(cal, 'kinect12_to_world', info['scene_name'] + '.json'))['trans'])
    if view != 'master':
        sub2main = np.asarray(read_json(os.path.join(cal, f'kinect_{EGOBODY_SUB_KINECT[view]}to12_color.json'))['trans'])
        cam2world = np.matmul(master2world, sub2main)
    else:
        cam2world = master2world
    return (cam2world, master2world) if return_master else cam2world


def read_prox_recording(init_root, base_dir, recording_name, joints_num=22):
    """dataloader_video.py:95-158: everything `read_data_prox` takes from the disk."""
    fitting_dir = os.path.join(init_root, recording_name, 'results')
    scene_name = recording_name.split('_')[0]
    frame_names = sorted(os.listdir(fitting_dir))
    kp_dir = os.path.join(base_dir, 'keypoints_openpose', recording_name)
    return {
        'scene_name': scene_name, 'frame_names': frame_names, 'params': read_fittings(fitting_dir, frame_names),
        'cam2world': read_cam2world('prox', base_dir, recording_name),
        'color_cam': read_json(os.path.join(base_dir, 'calibration', 'Color.json')),
        'keypoints': np.asarray([read_keypoints(os.path.join(kp_dir, n + '_keypoints.json'), joints_num) for n in frame_names]),
        'mask_joint': np.load(os.path.join(base_dir, 'mask_joint', recording_name, 'mask_joint.npy')),
    }


def read_egobody_info(base_dir, recording_name):
    """egobody_rohm_info.csv + data_splits.csv (:185-227) -> the recording's row and the root of its ground-truth fittings."""
    with open(os.path.join(base_dir, 'egobody_rohm_info.csv'), newline='') as f:
        rows = [r for r in csv.DictReader(f) if r['recording_name'] == recording_name]
    if not rows:
        raise KeyError(f'{recording_name} is not in egobody_rohm_info.csv')
    row = rows[-1]
    info = {'view': row['view'], 'body_idx': int(row['target_idx']), 'scene_name': row['scene_name'],
            'gender_gt': row['target_gender']}
    split = None
    with open(os.path.join(base_dir, 'data_splits.csv'), newline='') as f:
        for r in csv.DictReader(f):
            for name in ('train', 'val', 'test'):
                if split is None and r.get(name) == recording_name:
                    split = name
    if split is None:
        raise KeyError(f'{recording_name} not in all splits')
    interactee_idx = int(row['body_idx_fpv'].split(' ')[0])
    role = 'interactee' if info['body_idx'] == interactee_idx else 'camera_wearer'
    info['fitting_gt_root'] = os.path.join(base_dir, f'smplx_{role}_{split}', recording_name, f"body_idx_{info['body_idx']}")
    return info


def read_egobody_recording(init_root, base_dir, recording_name, joints_num=22):
    """dataloader_video.py:184-343: everything `read_data_egobody` takes from the disk."""
    info = read_egobody_info(base_dir, recording_name)
    view, idx = info['view'], info['body_idx']
    fitting_dir = os.path.join(init_root, recording_name, f'body_idx_{idx}', 'results')
    frame_names = sorted(os.listdir(fitting_dir))
    cam2world, master2world = read_cam2world('egobody', base_dir, recording_name, info, return_master=True)
    kp_dir = os.path.join(base_dir, 'keypoints_cleaned', recording_name, view)
    info.update({
        'frame_names': frame_names, 'params': read_fittings(fitting_dir, frame_names),
        'params_gt': read_fittings(os.path.join(info['fitting_gt_root'], 'results'), frame_names),
        'cam2world': cam2world, 'master2world': master2world,
        'color_cam': read_json(os.path.join(base_dir, 'kinect_cam_params', f'kinect_{view}', 'Color.json')),
        'keypoints': np.asarray([read_keypoints(os.path.join(kp_dir, n + '_keypoints.json'), joints_num, idx) for n in frame_names]),
        'mask_joint': np.load(os.path.join(base_dir, 'mask_joint', recording_name, view, 'mask_joint.npy')),
    })
    return info


def _floor_table(dataset, floor_heights, rohm_root):
    if floor_heights is not None:
        if isinstance(floor_heights, (str, os.PathLike)):
            floor_heights = read_json(floor_heights)
        return {str(k): float(v) for k, v in dict(floor_heights).items()}
    if rohm_root:
        from ..evaluation import read_floor_heights
        return read_floor_heights(rohm_root, dataset)
    return None


def _dev32(x, device):
    if torch.is_tensor(x):
        return x.to(device=device, dtype=torch.float32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(device)


def _body_model(body_model_path, gender, device):
    """An injected nn.Module (used for every gender), an SMPLX_*.npz file, or a model directory."""
    from ..body_model import SMPLXLayer
    if isinstance(body_model_path, torch.nn.Module):
        return body_model_path.to(device)
    path, name = str(body_model_path), f'SMPLX_{gender.upper()}.npz'
    cands = [os.path.join(path, name), os.path.join(path, 'smplx', name)]
    if path.endswith('.npz'):
        cands.insert(0, os.path.join(os.path.dirname(path), name) if gender != 'neutral' else path)
    for cand in cands:
        if os.path.isfile(cand):
            return SMPLXLayer.from_npz(cand).to(device)
    try:
        import smplx
    except ImportError:
        raise FileNotFoundError(f'no {name} under {body_model_path} (and smplx is not installed)') from None
    return smplx.create(model_path=path, model_type='smplx', gender=gender, flat_hand_mean=True, use_pca=False).to(device)


# ---- the dataset --------------------------------------------------------------------------------------------------------------
class DataloaderVideo(data.Dataset):
    def __init__(self, dataset='prox', init_root='', base_dir='', body_model_path='', recording_name='',
                 use_scene_floor_height=False, repr_abs_only=False, task='traj', overlap_len=2, clip_len=150, joints_num=22,
                 logdir=None, device='cuda', floor_heights=None, rohm_root=None):
        if dataset not in ('prox', 'egobody'):
            raise ValueError(f'dataset {dataset!r} not defined')
        self._setup(dataset, task, repr_abs_only, clip_len, overlap_len, joints_num, logdir, device, use_scene_floor_height)
        self.init_root, self.base_dir, self.recording_name = init_root, base_dir, recording_name
        self.up_axis, self.undistort, self.image_width = ('z', True, 1920) if dataset == 'prox' else ('y', False, 1920)

        read = read_prox_recording if dataset == 'prox' else read_egobody_recording
        rec = read(init_root, base_dir, recording_name, joints_num)
        self._camera(rec)
        if dataset == 'egobody':
            self.view, self.body_idx, self.gender_gt = rec['view'], rec['body_idx'], rec['gender_gt']
            self.fitting_gt_root = rec['fitting_gt_root']
        table = _floor_table(dataset, floor_heights, rohm_root)
        self.scene_floor_height = table[self.scene_name] if table is not None else None
        if use_scene_floor_height and self.scene_floor_height is None:
            raise ValueError('use_scene_floor_height needs floor_heights= or rohm_root=')
        self._stats_and_model(logdir, body_model_path)
        self._build(rec, body_model_path)

    def _setup(self, dataset, task, repr_abs_only, clip_len, overlap_len, joints_num, logdir, device, use_scene_floor_height):
        """What does not depend on where the recording comes from (data_loaders/track.py starts here too)."""
        if task not in ('traj', 'pose'):
            raise ValueError("task should be in ['traj', 'pose']")
        if joints_num != 22:
            raise ValueError('the motion representation is defined for joints_num = 22')
        self.dataset, self.task, self.repr_abs_only = dataset, task, repr_abs_only
        self.clip_len, self.clip_overlap_len, self.joints_num = clip_len, overlap_len, joints_num
        self.logdir = logdir
        self.use_scene_floor_height = use_scene_floor_height
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise _lib.RohmHipError('DataloaderVideo builds its clips on an AMD GPU; there is no CPU fallback')
        self.openpose_to_smpl = OPENPOSE_TO_SMPL[0:joints_num]

        if not repr_abs_only:
            self.traj_repr_name_list = ['root_rot_angle', 'root_rot_angle_vel', 'root_l_pos', 'root_l_vel', 'root_height',
                                        'smplx_rot_6d', 'smplx_rot_vel', 'smplx_trans', 'smplx_trans_vel']
        else:
            self.traj_repr_name_list = ['root_rot_angle', 'root_l_pos', 'root_height', 'smplx_rot_6d', 'smplx_trans']
        self.local_repr_name_list = ['local_positions', 'local_vel', 'smplx_body_pose_6d', 'smplx_betas', 'foot_contact']
        self.body_feat_dim = sum(REPR_DIM_DICT.values())
        self.traj_feat_dim = sum(REPR_DIM_DICT[k] for k in self.traj_repr_name_list)
        self.pose_feat_dim = sum(REPR_DIM_DICT[k] for k in self.local_repr_name_list)

    def _camera(self, rec):
        self.scene_name, self.color_cam = rec['scene_name'], rec['color_cam']
        # dataloader_video.py:102-104, :252-254: what PoseNet's 2-D guidance reads of its dataset (posenet.py:296)
        cam2world = torch.from_numpy(np.asarray(rec['cam2world'], dtype=np.float64)).float().to(self.device)
        self.cam_R, self.cam_t = cam2world[:3, :3].reshape([3, 3]), cam2world[:3, 3].reshape([1, 3])

    def _stats_and_model(self, logdir, body_model_path):
        self.Mean_dict, self.Std_dict, self.Mean, self.Std = read_stats(logdir)
        self.smplx_neutral = _body_model(body_model_path, 'neutral', self.device)

    def _build(self, rec, body_model_path, starts=None):
        """rec['params'] / ['keypoints'] / ['mask_joint'] are host arrays or device tensors; `starts`: explicit window starts
        (data_loaders/track.py) instead of the reference's windows."""
        dev, L, ov = self.device, self.clip_len, self.clip_overlap_len
        n_frames = len(rec['frame_names'])
        joints_world, smplx_world = frames.frames_to_world(self.smplx_neutral, rec['params'], rec['cam2world'], dev)
        built = clips.build_clips(joints_world, smplx_world, L, ov, up_axis=self.up_axis, starts=starts,
                                  preset_floor_height=self.scene_floor_height if self.use_scene_floor_height else None,
                                  stats=(self.Mean, self.Std))
        n = self.n_samples = int(built['repr'].shape[0])
        idx = built['starts'].long()[:, None] + torch.arange(L, device=dev)[None]                  # [C, L] frame indices
        kp_host = rec['keypoints'][:, 0:self.joints_num]
        kp, mask = _dev32(kp_host, dev), _dev32(rec['mask_joint'][:n_frames], dev)
        joint_vis, vec_vis = clips.visibility_masks(kp, mask, L, ov, starts=starts)
        if self.undistort:
            kp = clips.undistort_keypoints(kp, self.color_cam['camera_mtx'], self.color_cam['k'], self.image_width)
        f32 = dict(device=dev, dtype=torch.float32)
        focal = torch.tensor([self.color_cam['f'][0], self.color_cam['f'][1]], **f32)
        center = torch.tensor([self.color_cam['c'][0], self.color_cam['c'][1]], **f32)
        world_clips = smplx_world[idx]                                                              # [C, L, 79]
        dv = {'motion_repr_noisy': built['repr'], 'noisy_joints': built['cano_joints'],
              'noisy_joints_scene_coord': joints_world[idx]}
        if self.dataset == 'egobody':
            gt_model = _body_model(body_model_path, self.gender_gt, dev)
            dv['gt_joints_scene_coord'] = frames.frames_to_world(gt_model, rec['params_gt'], rec['master2world'], dev)[0][idx]
        dv.update({'transf_matrix': built['transf_matrix'], 'global_orient': built['global_orient'], 'transl': built['transl'],
                   'betas': world_clips[..., 6:16].float(), 'body_pose': world_clips[..., 16:79].float(),
                   'focal_length': focal[None].repeat(n, 1), 'camera_center': center[None].repeat(n, 1),
                   'keypoints_2d': kp[idx], 'mask_joint_vis': joint_vis, 'mask_vec_vis': vec_vis})
        if self.task == 'traj':
            full = built['repr']
            dv['cond'] = full[..., list(ABS_TRAJ_CH)].contiguous() if self.repr_abs_only else full[..., 0:self.traj_feat_dim]
            dv['control_cond'] = full[..., -self.pose_feat_dim:]
        self._device_data = {k: v.contiguous() for k, v in dv.items()}
        # one device -> host copy for the items
        flat = torch.cat([v.reshape(-1) for v in self._device_data.values()]).cpu().numpy()
        self._host, off = {}, 0
        for k, v in self._device_data.items():
            self._host[k] = flat[off:off + v.numel()].reshape(tuple(v.shape))
            off += v.numel()
        if self.dataset == 'egobody':          # not undistorted: the items carry the file's values in the reference's dtype
            self._host['keypoints_2d'] = kp_host[idx.cpu().numpy()]
        starts = built['starts'].tolist()
        self.frame_name_list = [rec['frame_names'][s:s + L] for s in starts]

    def __getstate__(self):
        # what a DataLoader worker gets (spawn / forkserver): the host items only, nothing that lives on the device
        return {k: v for k, v in self.__dict__.items()
                if k not in ('_device_data', 'smplx_neutral', 'cam_R', 'cam_t') and not k.startswith('_rohm_stats_')}

    def __len__(self):
        return self.n_samples

    def __getitem__(self, index):
        h = self._host
        item = {k: h[k][index] for k in ('motion_repr_noisy', 'noisy_joints', 'noisy_joints_scene_coord')}
        if self.dataset == 'egobody':
            item['gt_joints_scene_coord'] = h['gt_joints_scene_coord'][index]
        item['transf_matrix'] = h['transf_matrix'][index]
        item['cano_smplx_params_dict'] = {k: h[k][index] for k in ('global_orient', 'transl', 'betas', 'body_pose')}
        item['frame_name'] = self.frame_name_list[index]
        item['focal_length'], item['camera_center'] = h['focal_length'][index], h['camera_center'][index]
        kp = h['keypoints_2d'][index]
        item['keypoints_2d'] = kp.astype(np.float64) if self.dataset == 'prox' else kp
        item['mask_joint_vis'], item['mask_vec_vis'] = h['mask_joint_vis'][index], h['mask_vec_vis'][index]
        if self.task == 'traj':
            item['cond'], item['control_cond'] = h['cond'][index], h['control_cond'][index]
        return item

    def batches(self, batch_size):
        """The collated batches of a `DataLoader(self, batch_size, shuffle=False)` as device tensors (views of the
        loader's tensors; `frame_name` is the [bs, clip_len] array the driver makes of it)."""
        d = self._device_data
        for a in range(0, self.n_samples, batch_size):
            b = min(a + batch_size, self.n_samples)
            batch = {k: v[a:b] for k, v in d.items() if k not in ('global_orient', 'transl', 'betas', 'body_pose')}
            batch['cano_smplx_params_dict'] = {k: d[k][a:b] for k in ('global_orient', 'transl', 'betas', 'body_pose')}
            batch['frame_name'] = np.asarray(self.frame_name_list[a:b])
            yield batch
