"""TEST INFRASTRUCTURE ONLY: a small synthetic PROX / EgoBody directory tree in the layout the reference's test-time
loader reads (data_loaders/dataloader_video.py:95-157, :184-343), as arrays (`synthetic_tree_arrays`, stored in
tests/golden/video_loader.npz) and written to disk from those arrays (`write_tree`)."""
import csv
import json
import os
import pickle

import numpy as np

from oracle import geometry as G
from rohm_amd.utils import synth

N_FRAMES, CLIP_LEN, OVERLAP = 20, 8, 2
EMPTY_FRAME = 6                         # the frame whose OpenPose file has no people
PARAM_SLICES = {'transl': (0, 3), 'global_orient': (3, 6), 'betas': (6, 16), 'body_pose': (16, 79)}
NAMES = {'prox': dict(recording_name='N0Sofa_00034_01', scene_name='N0Sofa'),
         'egobody': dict(recording_name='recording_20210907_S02_S01_01', scene_name='seminar_g110', view='sub_1',
                         target_idx=1, target_gender='female', body_idx_fpv='1 fpv', split='val')}


def _rigid(g, angle):
    m = np.eye(4)
    m[:3, :3] = synth._rodrigues_np(g.standard_normal((1, 3)) * angle)[0]
    m[:3, 3] = g.standard_normal(3) * 0.5
    return m


def _to_camera(world, cam2world):
    """World-frame [n,79] rows (global_orient, transl, betas, body_pose) -> camera-frame fitting results (float32, the
    pickles' order transl, global_orient, betas, body_pose)."""
    from scipy.spatial.transform import Rotation as R
    inv = np.linalg.inv(cam2world)
    go = R.from_matrix(inv[:3, :3] @ R.from_rotvec(world[:, 0:3]).as_matrix()).as_rotvec()
    tr = world[:, 3:6] @ inv[:3, :3].T + inv[:3, 3]
    return np.concatenate([tr, go, world[:, 6:16], world[:, 16:79]], axis=-1).astype(np.float32)


def _params(g, n, cam2world, up_axis):
    """Camera-frame fitting results [n,79] (float32) of `synth.synthetic_recording`'s body."""
    return _to_camera(synth.synthetic_recording(int(g.integers(1 << 20)), n, up_axis)[1], cam2world)


def tree_motion(g, n, up_axis):
    """World-frame parameters [n,79] of a body whose facing direction is WELL CONDITIONED.

    The loader tests compare a canonicalisation that starts from the device's float32 joints with one that starts from the
    oracle body model's: two float32 forward kinematics agree to about an ulp of the coordinates (1.2e-7 at 1-2 m), and
    the facing rotation of `cano_seq_smplx` turns a joint difference d into an angle ~ 2 d / |across_xy| and then into
    ~ angle x 1 m of position.  The synthetic body's hip and shoulder axes are short (0.13 m, 0.05 m: |across_xy| ~ 0.1 m), which
    puts that at the 5e-6 bar of the geometry; a constant offset on the spine / collar joints, found by a seeded
    random search, spreads the shoulders (|shoulder axis| >= 0.45 m is asserted), which keeps it an order of magnitude
    below.  On top: the rotation that lays the shoulder axis onto +x, a slow yaw (+-0.3 rad), body pose +-0.12 rad, a
    root drift of +-0.2 m."""
    bt = synth.synthetic_smplx_tensors(0)
    betas = (g.standard_normal((1, 10)) * 0.3).astype(np.float32).astype(np.float64)
    trials = 512
    off = np.zeros((trials, 63))
    for j in (3, 6, 9, 13, 14):
        off[:, (j - 1) * 3:j * 3] = g.uniform(-1.5, 1.5, size=(trials, 3))
    rest = synth._fk_np(bt, np.tile(np.eye(3), (trials, 1, 1)), off, np.repeat(betas, trials, 0), np.zeros((trials, 3)))
    sdr = rest[:, 17] - rest[:, 16]
    best = int(np.argmax(np.linalg.norm(sdr, axis=1)))
    a = sdr[best]
    assert np.linalg.norm(a) >= 0.45, np.linalg.norm(a)
    a = a / np.linalg.norm(a)
    ax = np.cross(a, [1.0, 0.0, 0.0])
    sn, cs = np.linalg.norm(ax), float(a[0])
    R0 = synth._rodrigues_np((ax / max(sn, 1e-12) * np.arctan2(sn, cs))[None])[0]
    t = np.arange(n) / 30.0

    def slow(tail, amp):
        f, ph = g.uniform(0.1, 0.5, size=tail), g.uniform(0, 2 * np.pi, size=tail)
        return amp * np.sin(2 * np.pi * f * t.reshape((n,) + (1,) * len(tail)) + ph)
    yaw = slow((), 0.3)
    Rz = np.zeros((n, 3, 3))
    Rz[:, 0, 0], Rz[:, 0, 1], Rz[:, 1, 0], Rz[:, 1, 1], Rz[:, 2, 2] = np.cos(yaw), -np.sin(yaw), np.sin(yaw), np.cos(yaw), 1.0
    U = np.eye(3) if up_axis == 'z' else np.array([[1.0, 0, 0], [0, 0, 1.0], [0, -1.0, 0]])
    from scipy.spatial.transform import Rotation as R
    go = R.from_matrix(U @ Rz @ R0).as_rotvec()
    body_pose = (off[best][None] + slow((63,), 0.12)).astype(np.float32).astype(np.float64)
    transl = (np.array([0.2, -0.1, 0.0]) + slow((3,), 0.2)) @ U.T
    return np.concatenate([go, transl, np.repeat(betas, n, 0), body_pose], axis=-1)


def synthetic_tree_arrays(dataset, seed=0):
    g = np.random.Generator(np.random.PCG64(seed + (17 if dataset == 'prox' else 29)))
    n = N_FRAMES
    out = {k: np.str_(v) if isinstance(v, str) else np.int64(v) for k, v in NAMES[dataset].items()}
    up_axis = 'z' if dataset == 'prox' else 'y'
    if dataset == 'prox':
        cam2world = _rigid(g, 0.3)
        out['cam2world'] = cam2world
    else:
        out['master2world'], out['sub2main'] = _rigid(g, 0.3), _rigid(g, 0.2)
        cam2world = out['master2world'] @ out['sub2main']
        out['params_gt'] = _to_camera(tree_motion(g, n, up_axis), out['master2world'])
    out['params'] = _to_camera(tree_motion(g, n, up_axis), cam2world)
    n_people = 1 if dataset == 'prox' else 2
    kp = np.concatenate([g.uniform(size=(n, n_people, 25, 2)) * np.array([1920., 1080.]), g.uniform(size=(n, n_people, 25, 1))], -1)
    out['keypoints'] = kp.astype(np.float32)
    present = np.ones(n, bool)
    present[EMPTY_FRAME] = False
    out['people_present'] = present
    out['mask_joint'] = (g.uniform(size=(n, 25)) > 0.3).astype(np.float64)
    out['frame_names'] = np.array([f's001_frame_{i + 1:05d}' for i in range(n)])
    out['cam_f'], out['cam_c'] = np.array([1060.53, 1060.38]), np.array([951.30, 536.77])
    out['cam_mtx'] = np.array([[1060.53, 0, 951.30], [0, 1060.38, 536.77], [0, 0, 1.0]])
    out['cam_k'] = np.array([0.05, -0.04, 0.001, -0.0008, 0.01])
    mean, std = synth.synthetic_stats(5)
    out['mean'], out['std'] = mean, std
    return out


def _dump_params(path, row):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'wb') as f:
        pickle.dump({k: row[None, a:b].copy() for k, (a, b) in PARAM_SLICES.items()}, f)


def _stats_dict(vec):
    out, off = {}, 0
    for name in G.REPR_LIST:
        out[name] = np.asarray(vec[off:off + G.REPR_DIM[name]])
        off += G.REPR_DIM[name]
    return out


def _json(path, obj):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(obj, f)


def write_tree(root, dataset, a):
    """Write the arrays of `synthetic_tree_arrays` (or the same keys of the fixture) as the reference's file layout under
    `root`; returns the three roots the loader's constructor takes."""
    init_root, base, logdir = (os.path.join(root, d) for d in ('init', 'base', 'log'))
    rec, scene = str(a['recording_name']), str(a['scene_name'])
    names = [str(s) for s in a['frame_names']]
    cam = {'f': a['cam_f'].tolist(), 'c': a['cam_c'].tolist(), 'camera_mtx': a['cam_mtx'].tolist(), 'k': a['cam_k'].tolist()}
    os.makedirs(logdir, exist_ok=True)
    for name, vec in (('AMASS_mean.pkl', a['mean']), ('AMASS_std.pkl', a['std'])):
        with open(os.path.join(logdir, name), 'wb') as f:
            pickle.dump(_stats_dict(vec), f)
    if dataset == 'prox':
        fit, mask_dir = os.path.join(init_root, rec, 'results'), os.path.join(base, 'mask_joint', rec)
        kp_dir = os.path.join(base, 'keypoints_openpose', rec)
        _json(os.path.join(base, 'cam2world', scene + '.json'), a['cam2world'].tolist())
        _json(os.path.join(base, 'calibration', 'Color.json'), cam)
    else:
        view, idx, split = str(a['view']), int(a['target_idx']), str(a['split'])
        fit = os.path.join(init_root, rec, f'body_idx_{idx}', 'results')
        mask_dir, kp_dir = os.path.join(base, 'mask_joint', rec, view), os.path.join(base, 'keypoints_cleaned', rec, view)
        gt = os.path.join(base, f'smplx_interactee_{split}', rec, f'body_idx_{idx}', 'results')
        cal = os.path.join(base, 'calibrations', rec, 'cal_trans')
        _json(os.path.join(cal, 'kinect12_to_world', scene + '.json'), {'trans': a['master2world'].tolist()})
        _json(os.path.join(cal, 'kinect_11to12_color.json'), {'trans': a['sub2main'].tolist()})
        _json(os.path.join(base, 'kinect_cam_params', f'kinect_{view}', 'Color.json'), cam)
        with open(os.path.join(base, 'egobody_rohm_info.csv'), 'w', newline='') as f:
            w = csv.writer(f)
            w.writerow(['recording_name', 'target_idx', 'target_gender', 'view', 'scene_name', 'body_idx_fpv'])
            w.writerow(['recording_20210101_S00_S00_00', 0, 'male', 'master', 'seminar_d78', '0 fpv'])
            w.writerow([rec, idx, str(a['target_gender']), view, scene, str(a['body_idx_fpv'])])
        with open(os.path.join(base, 'data_splits.csv'), 'w', newline='') as f:
            w = csv.writer(f)
            w.writerow(['train', 'val', 'test'])
            w.writerow(['recording_20210101_S00_S00_00', rec, 'recording_20210102_S00_S00_00'])
            w.writerow(['recording_20210103_S00_S00_00', '', ''])
        for i, name in enumerate(names):
            _dump_params(os.path.join(gt, name, '000.pkl'), a['params_gt'][i])
    os.makedirs(mask_dir, exist_ok=True)
    np.save(os.path.join(mask_dir, 'mask_joint.npy'), a['mask_joint'])
    for i, name in enumerate(names):
        _dump_params(os.path.join(fit, name, '000.pkl'), a['params'][i])
        people = [{'pose_keypoints_2d': [float(v) for v in p.reshape(-1)]} for p in a['keypoints'][i]] if a['people_present'][i] else []
        _json(os.path.join(kp_dir, name + '_keypoints.json'), {'version': 1.3, 'people': people})
    return {'init_root': init_root, 'base_dir': base, 'logdir': logdir}


def tree_arrays_from_fixture(g, dataset):
    """The `synthetic_tree_arrays` dict as stored in tests/golden/video_loader.npz."""
    prefix = f'{dataset}_tree_'
    return {k[len(prefix):]: g[k] for k in g.files if k.startswith(prefix)}
