"""TEST INFRASTRUCTURE ONLY: a numpy / scipy restatement of the reference's AMASS loader
(data_loaders/dataloader_amass.py) on top of oracle/rederive.py::get_repr_smplx, oracle/frames.py::noisy_clip_joints and
tests/clips_ref.py::canonicalize, plus the small synthetic AMASS tree of tests/golden/amass_loader.npz.  Pinned to the
reference's own loader by tests/test_amass_ref.py, so the GPU tests can use it at other shapes."""
import glob
import os

import numpy as np
from scipy.spatial.transform import Rotation as R

import clips_ref as CR
from oracle import frames as OF
from oracle import geometry as G
from oracle import rederive as RD
from rohm_amd.utils import synth

CLIP_LEN = 16
# dataset -> {sequence directory -> (seed of synth.synthetic_recording, frames)}: 40 frames give 2 train / 2 test clips
# (remainder dropped), 12 frames none (skipped), 33 frames 2 train clips and, after [1:-1], 1 test clip
TREE = {'SetA': {'walk': (31, 40), 'short': (32, 12)}, 'SetB': {'turn': (33, 33)}}
PARAM_NAMES = ('global_orient', 'transl', 'body_pose', 'betas')
NOISE_ORDER = ('transl', 'body_pose', 'betas', 'global_orient')          # dataloader_amass.py:159
STAGE1_STD = dict(noise_std_smplx_global_rot=1.0, noise_std_smplx_body_rot=1.0, noise_std_smplx_trans=0.01,
                  noise_std_smplx_betas=0.01)
STAGE2_STD = dict(noise_std_smplx_global_rot=2.0, noise_std_smplx_body_rot=2.0, noise_std_smplx_trans=0.03,
                  noise_std_smplx_betas=0.2)
SEP_STD = dict(noise_std_smplx_global_rot=0.01, noise_std_smplx_body_rot=0.01, noise_std_smplx_trans=0.002,
               noise_std_smplx_betas=0.01)
SEP_STD_JOINT = 1e-4
# numpy seeds of the fixture's cases a, b, d: chosen with `python scripts/make_golden_amass.py scan` so that the
# assertions of that script hold (few contact decisions near a threshold, both contact values in case a's noisy clips)
SEED_A, SEED_B, SEED_D = 0, 2, 0
ABS_TRAJ_CH = [0, 2, 3, 6, 7, 8, 9, 10, 11, 12, 16, 17, 18]
TRAJ_DIM, POSE_DIM = 22, 272
GROUPS = {}
_o = 0
for _n in G.REPR_LIST:
    GROUPS[_n] = (_o, _o + G.REPR_DIM[_n])
    _o += G.REPR_DIM[_n]
FOOT = ((7, 0.18), (10, 0.15), (8, 0.18), (11, 0.15))                   # contact channel order


# ---- the tree ---------------------------------------------------------------------------------------------------------
def tree_arrays():
    """{'<dataset>/<sequence>': (joints [n,25,3] float32, smplx [n,178] float64)} as preprocessing_amass.py writes them."""
    out = {}
    for ds, seqs in TREE.items():
        for name, (seed, n) in seqs.items():
            jw, world = synth.synthetic_recording(seed, n, 'z')
            joints = np.zeros((n, 25, 3), np.float32)
            joints[:, :22] = jw
            smplx = np.zeros((n, 178))
            smplx[:, :79] = world
            out[f'{ds}/{name}'] = (joints, smplx)
    return out


def write_tree(root, arrays):
    for key, (joints, smplx) in arrays.items():
        for sub, a in (('pose_data_fps_30', joints), ('smpl_data_fps_30', smplx)):
            d = os.path.join(root, sub, key)
            os.makedirs(d, exist_ok=True)
            np.save(os.path.join(d, 'poses.npy'), a)
    return root


def read_clips(root, datasets, split, clip_len):
    """`divide_clip`: the list of (joints [L,22,3] float32, params dict of float64) clips."""
    clips = []
    for ds in datasets:
        for path in sorted(glob.glob(os.path.join(root, 'pose_data_fps_30', ds, '*/*.npy'))):
            seq, name = path.split('/')[-2:]
            joints, smplx = np.load(path), np.load(os.path.join(root, 'smpl_data_fps_30', ds, seq, name))
            if split == 'test':
                joints, smplx = joints[1:-1], smplx[1:-1]
            for i in range(int(len(joints) / clip_len) if len(joints) >= clip_len else 0):
                s = slice(clip_len * i, clip_len * (i + 1))
                clips.append((joints[s, :22], CR.split_world(smplx[s, :79])))
    return clips


# ---- noise ------------------------------------------------------------------------------------------------------------
def euler_zxy(rotvec):
    """`R.from_rotvec(v).as_euler('zxy', degrees=True)` written out: R = Ry(e2) Rx(e1) Rz(e0)."""
    M = R.from_rotvec(rotvec).as_matrix()
    return np.degrees(np.stack([np.arctan2(M[:, 1, 0], M[:, 1, 1]), np.arcsin(np.clip(-M[:, 1, 2], -1, 1)),
                                np.arctan2(M[:, 0, 2], M[:, 2, 2])], -1))


def perturb_rotvec(rotvec, noise_deg):
    """Euler-space noise of dataloader_amass.py:170-189 on rotation vectors [n,3]."""
    ang = R.from_rotvec(rotvec).as_euler('zxy', degrees=True)
    return R.from_euler('zxy', ang + noise_deg, degrees=True).as_rotvec()


def draw_noise(T, stds):
    """One clip's draws in the reference's order and shapes (body_pose returned as [T,21,3])."""
    out = {}
    for name in NOISE_ORDER:
        shape = {'transl': (T, 3), 'betas': (T, 10), 'global_orient': (T, 3), 'body_pose': (T * 21, 3)}[name]
        out[name] = np.random.normal(loc=0.0, scale=stds[name], size=shape)
    out['body_pose'] = out['body_pose'].reshape(T, 21, 3)
    return out


def std_dict(kw):
    return {'global_orient': kw['noise_std_smplx_global_rot'], 'transl': kw['noise_std_smplx_trans'],
            'body_pose': kw['noise_std_smplx_body_rot'], 'betas': kw['noise_std_smplx_betas']}


def perturb_params(params, noise):
    T = len(params['transl'])
    return {'transl': params['transl'] + noise['transl'], 'betas': params['betas'] + noise['betas'],
            'global_orient': perturb_rotvec(params['global_orient'], noise['global_orient']),
            'body_pose': perturb_rotvec(params['body_pose'].reshape(-1, 3), noise['body_pose'].reshape(-1, 3)).reshape(T, 21, 3)}


def euler_margins(params, noisy):
    """(smallest distance in degrees of a clean or noisy Euler middle angle to +-90, smallest distance in rad of a noisy
    rotation's angle to pi) over lists of parameter dicts."""
    mid, ang = np.inf, np.inf
    for p, q in zip(params, noisy):
        for k in ('global_orient', 'body_pose'):
            a, b = np.asarray(p[k]).reshape(-1, 3), np.asarray(q[k]).reshape(-1, 3)
            for v in (a, b):
                mid = min(mid, (90 - np.abs(R.from_rotvec(v).as_euler('zxy', degrees=True)[:, 1])).min())
            ang = min(ang, (np.pi - np.linalg.norm(b, axis=-1)).min())
    return float(mid), float(ang)


# ---- representation ------------------------------------------------------------------------------------------------------
def full_repr(positions, params):
    p = dict(params)
    p['body_pose'] = np.asarray(p['body_pose']).reshape(len(p['transl']), 63)
    return RD.full_repr(RD.get_repr_smplx(positions, p))


def near_threshold(joints, rel=1e-2):
    """[C, T-1, 4] bool: contact decisions of `foot_detect` within a relative `rel` of the velocity or height threshold."""
    p = np.asarray(joints, np.float64)
    out = []
    for j, h in FOOT:
        sq = ((p[:, 1:, j] - p[:, :-1, j]) ** 2).sum(-1)
        out.append((np.abs(sq / 5e-5 - 1) < rel) | (np.abs(p[:, :-1, j, 2] / h - 1) < rel))
    return np.stack(out, -1)


def dataset_stats(clean_repr):
    """dataloader_amass.py:251-263 on the stacked clean representation [n, T-1, 294] (float64 in, float32 out)."""
    flat = np.asarray(clean_repr).reshape(-1, 294)
    mean, std = {}, {}
    for name, (a, b) in GROUPS.items():
        mean[name] = flat[:, a:b].mean(axis=0).astype(np.float32)
        std[name] = flat[:, a:b].std(axis=0).astype(np.float32)
        if name == 'foot_contact':
            mean[name][...] = 0.0
            std[name][...] = 1.0
        elif name != 'smplx_betas':
            std[name][...] = std[name].mean()
    return mean, std


# ---- the loader ---------------------------------------------------------------------------------------------------------------
class Loader:
    """The reference's DataloaderAMASS, restated.  body_model: oracle.geometry.BodyModel.  stats: (Mean_dict, Std_dict)
    for split 'test'."""

    def __init__(self, root, body_model, amass_datasets, split='train', spacing=1, repr_abs_only=False, input_noise=False,
                 sep_noise=False, noise_std_joint=0.0, noise_std_smplx_global_rot=0.0, noise_std_smplx_body_rot=0.0,
                 noise_std_smplx_trans=0.0, noise_std_smplx_betas=0.0, load_noise=False, loaded_smplx_noise_dict=None,
                 task='traj', clip_len=150, stats=None):
        self.task, self.repr_abs_only, self.input_noise, self.sep_noise = task, repr_abs_only, input_noise, sep_noise
        self.noise_std_joint, self.spacing, self.clip_len = noise_std_joint, spacing, clip_len
        self.stds = std_dict(dict(noise_std_smplx_global_rot=noise_std_smplx_global_rot, noise_std_smplx_body_rot=noise_std_smplx_body_rot,
                                  noise_std_smplx_trans=noise_std_smplx_trans, noise_std_smplx_betas=noise_std_smplx_betas))
        clips = read_clips(root, amass_datasets, split, clip_len)
        self.n_samples = len(clips)
        self.joints_clean, self.params, self.transf, self.repr_clean = [], [], [], []
        self.noise, self.params_noisy, self.joints_noisy, self.repr_noisy = [], [], [], []
        for i in range(0, self.n_samples, spacing):
            cano, cp, tm = CR.canonicalize(*clips[i], 'z')
            if input_noise and not sep_noise:
                if load_noise:
                    nz = {k: np.asarray(loaded_smplx_noise_dict[k][i * spacing]) for k in NOISE_ORDER}
                else:
                    nz = draw_noise(clip_len, self.stds)
                noisy = perturb_params(cp, nz)
                jn = OF.noisy_clip_joints(body_model, {k: np.asarray(v).reshape(clip_len, -1) for k, v in noisy.items()})
                self.noise.append(nz)
                self.params_noisy.append(noisy)
                self.joints_noisy.append(jn)
                self.repr_noisy.append(full_repr(jn, noisy))
            self.joints_clean.append(cano)
            self.params.append(cp)
            self.transf.append(tm)
            self.repr_clean.append(full_repr(cano, cp))
        self.repr_clean = np.asarray(self.repr_clean)
        self.Mean_dict, self.Std_dict = dataset_stats(self.repr_clean) if split == 'train' else stats
        self.Mean = np.concatenate([self.Mean_dict[k] for k in self.Mean_dict], axis=-1)
        self.Std = np.concatenate([self.Std_dict[k] for k in self.Std_dict], axis=-1)

    def __len__(self):
        return self.n_samples // self.spacing

    def __getitem__(self, index):
        clean = self.repr_clean[index]
        item = {'motion_repr_clean': None}                  # the reference's key order
        if self.input_noise:
            if self.sep_noise:
                p = self.params[index]
                noisy = {k: p[k] + np.random.normal(loc=0.0, scale=self.stds[k], size=p[k].shape) for k in PARAM_NAMES}
                pos = self.joints_clean[index]
                pos = (pos + np.random.normal(loc=0.0, scale=self.noise_std_joint, size=pos.shape)).astype(np.float32)
                rep = full_repr(pos, noisy)
            else:
                pos, rep = self.joints_noisy[index], self.repr_noisy[index].copy()
            item['noisy_joints'] = pos
            if self.task == 'pose':
                rep[:, 0:TRAJ_DIM if not self.repr_abs_only else 13] = clean[:, 0:TRAJ_DIM if not self.repr_abs_only else 13]
        else:
            rep = clean.copy()
        item['motion_repr_clean'] = ((clean - self.Mean) / self.Std).astype(np.float32)
        item['motion_repr_noisy'] = ((rep - self.Mean) / self.Std).astype(np.float32)
        if self.task == 'traj':
            t = item['motion_repr_noisy']
            item['cond'] = t[:, ABS_TRAJ_CH] if self.repr_abs_only else t[:, 0:TRAJ_DIM]
            item['control_cond'] = item['motion_repr_clean'][:, -POSE_DIM:]
        return item


# ---- the fixture ----------------------------------------------------------------------------------------------------------------
def fixture_tree(g):
    """tests/golden/amass_loader.npz -> the arrays `write_tree` takes (padded to [n,25,3] / [n,178])."""
    out = {}
    for key in g.files:
        if key.startswith('tree_') and key.endswith('_joints'):
            name = key[len('tree_'):-len('_joints')]
            j, s = g[key], g[f'tree_{name}_smplx']
            joints = np.zeros((len(j), 25, 3), np.float32)
            joints[:, :22] = j
            smplx = np.zeros((len(s), 178))
            smplx[:, :79] = s
            out[name.replace('__', '/')] = (joints, smplx)
    return out


def fixture_stats(g):
    import pickle
    return pickle.loads(g['mean_pkl'].tobytes()), pickle.loads(g['std_pkl'].tobytes())


def fixture_params(g, prefix, n):
    """[{name: array}] per clip from the arrays `<prefix><name>` of the fixture."""
    return [{k: g[prefix + k][i] for k in PARAM_NAMES} for i in range(n)]


def rows79(params):
    """A parameter dict -> [T,79] rows (global_orient, transl, betas, body_pose)."""
    T = len(params['transl'])
    return np.concatenate([np.asarray(params[k], np.float64).reshape(T, -1) for k in ('global_orient', 'transl', 'betas', 'body_pose')], -1)


def joint_widening(joints_noisy, params_noisy, eps=5e-6, draws=8, seed=0):
    """Largest change per REPR_LIST group (de-normalised units, contact left out) of the representation when float32
    joints [C,T,22,3] move by uniform +-eps, over `draws` draws (numpy PCG64 `seed`)."""
    g = np.random.Generator(np.random.PCG64(seed))
    base = [full_repr(j, p) for j, p in zip(joints_noisy, params_noisy)]
    worst = {k: 0.0 for k in G.REPR_LIST if k != 'foot_contact'}
    for _ in range(draws):
        for j, p, b in zip(joints_noisy, params_noisy, base):
            moved = (np.asarray(j, np.float64) + g.uniform(-eps, eps, size=j.shape)).astype(np.float32)
            d = np.abs(full_repr(moved, p) - b)
            for k in worst:
                lo, hi = GROUPS[k]
                worst[k] = max(worst[k], float(d[:, lo:hi].max()))
    return worst


def widened_limits(ref, joints, widening, tol=2e-5, local_factor=4 * 0.0112):
    """`clips_ref.repr_limits` (the `_close` rule of tests/test_gpu_clips.py) plus 4x the measured `widening` per group."""
    lim = CR.repr_limits(ref, np.asarray(joints, np.float64), None, tol, local_factor)
    for k, w in widening.items():
        lo, hi = GROUPS[k]
        lim[..., lo:hi] += 4 * w
    return lim


# joint_widening of the fixture's noisy joints (cases a and b, the larger of the two; eps 5e-6, 8 draws, seed 0), measured
# on the CPU and re-measured by tests/test_amass_ref.py::test_joint_widening_measurement.  Groups made of the parameters
# alone do not move.
JOINT_WIDENING = {'root_rot_angle': 8.166e-05, 'root_rot_angle_vel': 1.070e-04, 'root_l_pos': 5.000e-06, 'root_l_vel': 1.405e-05,
                  'root_height': 4.992e-06, 'smplx_rot_6d': 0.0, 'smplx_rot_vel': 0.0, 'smplx_trans': 0.0, 'smplx_trans_vel': 0.0,
                  'local_positions': 4.397e-05, 'local_vel': 2.133e-05, 'smplx_body_pose_6d': 0.0, 'smplx_betas': 0.0}
