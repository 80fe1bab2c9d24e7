"""TEST INFRASTRUCTURE ONLY: the seeded inputs of tests/golden/drivers.npz (shared with scripts/make_golden_drivers.py, which
feeds them to the reference scripts' own tails) and a numpy restatement of what the tails compute around the joint recovery:
the de-normalisation (test_amass_full.py:387-396) and the trajectory report (test_trajnet.py:221-263, :333-366).  float32
numpy throughout, in the scripts' order, so the restatement is compared bit for bit."""
import numpy as np
import torch

from rohm_amd.utils import synth

BATCHES = (2, 1)          # clips per batch: every tail runs on two batches, the last one smaller (drop_last=False)
ABS_CH = [0, 2, 3, 6, 7, 8, 9, 10, 11, 12, 16, 17, 18]
REPORT_ERR = ['root_rot_err_rec'] + [f'root_{x}_err_rec_from_{r}' for r in ('abs_traj', 'rel_traj', 'smpl') for x in 'xyz']
REPORT_JITTER = ['root_pos_jitter_' + k for k in ('clean', 'noisy', 'rec_from_abs_traj', 'rec_from_rel_traj', 'rec_from_smpl')]
JOINT_NAMES = ('clean', 'noisy', 'rec_from_abs_traj', 'rec_from_rel_traj', 'rec_from_smpl')


def stats(seed=0):
    return synth.synthetic_stats(seed)


def _noise(seed, *shape):
    return torch.from_numpy(np.random.Generator(np.random.PCG64(seed)).standard_normal(shape).astype(np.float32))


def motion(seed, B, T, st):
    """Normalised [B, 294, 1, T]."""
    return synth.plausible_motion(seed, B, T, *st)


def rows(x):
    """[B, 294, 1, T] -> contiguous [B, T, 294]."""
    return x[:, :, 0].permute(0, 2, 1).contiguous()


def amass_inputs(i, st, T=15):
    """Batch i of the test_amass_full.py tail: what the loop leaves behind (all normalised)."""
    B = BATCHES[i]
    return {'clean': motion(100 + i, B, T, st),                         # test_batch_pose['motion_repr_clean'] [B, 294, 1, T]
            'rec': motion(110 + i, B, T, st),                           # val_output_pose [B, 294, 1, T]
            'noisy': rows(motion(120 + i, B, T, st)),                   # test_batch_pose['motion_repr_noisy'] [B, T, 294]
            'traj_noisy_full': rows(motion(130 + i, B, T + 1, st))[:, :, 0:22].contiguous()}      # [B, T + 1, 22]


def rows_large_inputs(st, B=3, T=143):
    return {'clean': motion(200, B, T, st), 'rec': motion(201, B, T, st), 'noisy': rows(motion(202, B, T + 1, st)),
            'traj_noisy_full': rows(motion(203, B, T + 1, st))[:, :, 0:22].contiguous()}


def posenet_inputs(i, st, T=16):
    B = BATCHES[i]
    return {'clean': motion(300 + i, B, T, st), 'rec': motion(310 + i, B, T, st), 'noisy': rows(motion(320 + i, B, T, st))}


def prox_inputs(i, st, dataset, T=15):
    B = BATCHES[i]
    g = np.random.Generator(np.random.PCG64(400 + i))
    f = lambda *sh: torch.from_numpy(g.standard_normal(sh).astype(np.float32))      # noqa: E731
    return {'noisy': motion(410 + i, B, T, st),                         # test_batch_pose['motion_repr_noisy'] [B, 294, 1, T]
            'rec': motion(420 + i, B, T, st),                           # val_output_joint
            'transf_matrix': f(B, 4, 4), 'noisy_joints_scene_coord': f(B, T + 2, 22, 3), 'gt_joints_scene_coord': f(B, T + 2, 22, 3),
            'mask_joint_vis': torch.from_numpy((g.random((B, T + 2, 22)) > 0.3).astype(np.float32)),
            'frame_name': np.array([[f'{dataset}_b{i}_c{c}_f{t:03d}' for t in range(T + 2)] for c in range(B)])}


def trajnet_inputs(i, st, T, body_tensors):
    B = BATCHES[i]
    clean = synth.walking_motion(500 + i, B, T, *st, body_tensors)      # [B, T, 294]
    return {'clean': clean, 'noisy': clean + 0.05 * _noise(510 + i, B, T, 294),
            'val_output': clean[..., ABS_CH] + 0.02 * _noise(520 + i, B, T, 13)}


# ---- restatements ------------------------------------------------------------------------------------------------------------
def denorm(x, mean, std):
    """`x * Std + Mean` of the scripts: float32 numpy, a rounded product and a rounded sum."""
    x = np.asarray(x, dtype=np.float32)
    return x * np.asarray(std, np.float32) + np.asarray(mean, np.float32)


def amass_denorm(inp, st, T=None):
    """(motion_repr_clean, motion_repr_rec, motion_repr_noisy) of test_amass_full.py:387-396."""
    mean, std = st
    clean, rec = rows(inp['clean']).numpy(), rows(inp['rec']).numpy()
    T = clean.shape[1] if T is None else T
    noisy = inp['noisy'][:, 0:T].numpy().copy()
    noisy[:, :, 0:22] = inp['traj_noisy_full'].numpy()[:, 0:T, :]
    return denorm(clean, mean, std), denorm(rec, mean, std), denorm(noisy, mean, std)


def traj_report(joints, rot_clean, rot_rec, fps=30):
    """test_trajnet.py:221-263 for all clips at once.  joints: five [n, T, 22, 3] (or [n, T, 1, 3]) float32 arrays in JOINT_NAMES'
    order; rot_*: [n, T] channel 0 of the de-normalised representations.  Returns (err [n, 10, T], jitter [n, 5, T - 3]) float32
    and their float64 per-clip sums [n, 15]."""
    p = [np.asarray(j, np.float32)[:, :, 0] for j in joints]
    err = [np.abs(np.asarray(rot_rec, np.float32) * 2 - np.asarray(rot_clean, np.float32) * 2)]
    for r in (2, 3, 4):
        for x in range(3):
            err.append(np.abs(p[r][:, :, x] - p[0][:, :, x]))
    jit = []
    for q in p:
        j = (q[:, 3:] - 3 * q[:, 2:-1] + 3 * q[:, 1:-2] - q[:, :-3]) * (fps ** 3)
        jit.append(np.linalg.norm(j, axis=-1))
    err, jit = np.stack(err, axis=1), np.stack(jit, axis=1)
    assert err.dtype == np.float32 and jit.dtype == np.float32
    sums = np.concatenate([err.astype(np.float64).sum(axis=2), jit.astype(np.float64).sum(axis=2)], axis=1)
    return err, jit, sums
