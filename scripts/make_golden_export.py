"""Golden vectors of the export step -> tests/golden/export.npz.

Inputs: the three clips (7 rows each) the reference's own DataloaderVideo made of the synthetic PROX tree
(tests/golden/video_loader.npz: 20 frames, clip_len 8, overlap 2), de-normalised, with seeded noise on the 6-D rotation
channels so that they are no longer orthonormal (a network's output is not), and a synthetic body model of 419 vertices.

Outputs, all from the reference's own functions:
  * `recover_from_repr_smpl(..., 'smplx_params', return_verts=True)`: canonical joints and vertices; the axis-angle parameter
    dict it builds inside is recomputed with its `rot6d_to_rotmat` / `rotation_matrix_to_angle_axis`;
  * `update_globalRT_for_smplx(params, inv(trans_scene2cano), delta_T=pelvis)`: scene-frame global_orient / transl;
  * `points_coord_trans(verts, inv(trans_scene2cano))`: scene-frame vertices (every third vertex is stored).
The function reshapes its vertices to 10 475 per frame: the 21 rows are padded to 25 and passed as one sequence, 25 x 419 =
10 475, and split again afterwards.

The restatement (tests/export_ref.py) is run on the same inputs; its largest differences from the reference -- the reference
computes its axis-angles and its body model in float32 -- are printed and stored as `measured_ref_error_*`; the tests' bars
are 4 x these.

The reference is imported through oracle.refload; none of its text is here.  Needs a RoHM checkout at
oracle.refload.REF_ROOT; run once where it exists, commit only the .npz:
    python scripts/make_golden_export.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle import geometry as G  # noqa: E402
from oracle import refload  # noqa: E402
from rohm_amd.utils import synth  # noqa: E402
import export_ref as ER  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
NUM_VERTS, VERT_STEP, NOISE_SEED, NOISE_STD = 419, 3, 23, 0.05


def inputs():
    g = np.load(os.path.join(GOLD, 'video_loader.npz'))
    mean, std = g['prox_tree_mean'].astype(np.float32), g['prox_tree_std'].astype(np.float32)
    rep = np.stack([g[f'prox_pose_min_item{i}_motion_repr_noisy'] for i in range(3)]).astype(np.float32)
    transf = np.stack([g[f'prox_pose_min_item{i}_transf_matrix'] for i in range(3)]).astype(np.float32)
    rep = rep * std + mean
    rng = np.random.Generator(np.random.PCG64(NOISE_SEED))
    noise = (rng.standard_normal(rep.shape) * NOISE_STD).astype(np.float32)
    rot = np.zeros(294, bool)
    rot[ER.CH_ROT6D:ER.CH_ROT6D + 6] = rot[ER.CH_POSE6D:ER.CH_POSE6D + 126] = True
    rep[..., rot] += noise[..., rot]
    return rep, transf


def main():
    if not refload.available():
        raise SystemExit(f'needs the reference checkout at {refload.REF_ROOT}')
    sys.modules.setdefault('cv2', __import__('types').ModuleType('cv2'))
    ref = refload.load()
    mr, ou = ref.motion_repr, ref.other_utils
    tensors = synth.synthetic_smplx_tensors(0, num_verts=NUM_VERTS)
    body = G.BodyModel(tensors)
    rep, transf = inputs()
    C, T = rep.shape[:2]
    rows = rep.reshape(C * T, 294)
    pad = np.concatenate([rows, rows[:25 - C * T]])[None]                               # [1, 25, 294]
    data, off = {}, 0
    for name in ou.REPR_LIST:
        d = ou.REPR_DIM_DICT[name]
        data[name] = torch.from_numpy(pad[..., off:off + d])
        off += d
    with torch.no_grad():
        joints, verts = mr.recover_from_repr_smpl(data, recover_mode='smplx_params', smplx_model=body, return_verts=True)
        go = ref.konia.rotation_matrix_to_angle_axis(ref.quaternion.rot6d_to_rotmat(data['smplx_rot_6d'].reshape(-1, 6)))
        bp = ref.konia.rotation_matrix_to_angle_axis(
            ref.quaternion.rot6d_to_rotmat(data['smplx_body_pose_6d'].reshape(-1, 6))).reshape(-1, 63)
    n = C * T
    joints = joints.reshape(25, 22, 3).numpy()[:n]
    verts = verts.reshape(25, NUM_VERTS, 3).numpy()[:n]
    go, bp = go.numpy()[:n], bp.numpy()[:n]
    transl, betas = rows[:, ER.CH_TRANS:ER.CH_TRANS + 3], rows[:, ER.CH_BETAS:ER.CH_BETAS + 10]
    go_scene, tr_scene, verts_scene, joints_scene = [], [], [], []
    for c in range(C):
        s = slice(c * T, (c + 1) * T)
        inv = np.linalg.inv(transf[c])
        prm = {'global_orient': go[s].astype(np.float64), 'transl': transl[s].astype(np.float64), 'betas': betas[s], 'body_pose': bp[s]}
        new = ou.update_globalRT_for_smplx(prm, inv, delta_T=joints[s, 0] - transl[s])
        go_scene.append(new['global_orient'])
        tr_scene.append(new['transl'])
        verts_scene.append(ou.points_coord_trans(verts[s].reshape(-1, 3), inv).reshape(T, NUM_VERTS, 3))
        joints_scene.append(ou.points_coord_trans(joints[s].reshape(-1, 3), inv).reshape(T, 22, 3))
    go_scene, tr_scene = np.concatenate(go_scene), np.concatenate(tr_scene)
    verts_scene, joints_scene = np.concatenate(verts_scene), np.concatenate(joints_scene)

    # the restatement on the same inputs, and its distance from the reference
    fc, ft = np.repeat(np.arange(C), T), np.tile(np.arange(T), C)
    pelvis = ER.fold_pelvis(tensors)
    cano, contact = ER.export_params(rep, fc, ft, pelvis)
    scene, _ = ER.export_params(rep, fc, ft, pelvis, transf=transf)
    ref_rv = np.concatenate([go_scene.reshape(n, 1, 3), bp.reshape(n, 21, 3).astype(np.float64)], axis=1)
    got_rv = np.concatenate([scene[:, 0:3].reshape(n, 1, 3), scene[:, 16:79].reshape(n, 21, 3)], axis=1)
    err_mat = float(np.abs(ER.rodrigues(got_rv) - ER.rodrigues(ref_rv)).max())
    err_mat = max(err_mat, float(np.abs(ER.rodrigues(cano[:, 0:3]) - ER.rodrigues(go.astype(np.float64))).max()))
    m = ER.rot_component_mask(ref_rv)
    err_vec = float(np.abs(got_rv - ref_rv)[m].max())
    err_tr = float(np.abs(scene[:, 3:6] - tr_scene).max())
    body64 = G.BodyModel(tensors, dtype=torch.float64)
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    out = body64(betas=t64(scene[:, 6:16]), global_orient=t64(scene[:, 0:3]), body_pose=t64(scene[:, 16:79]), transl=t64(scene[:, 3:6]))
    err_v = float(np.abs(out.vertices.numpy() - verts_scene).max())
    err_j = float(np.abs(out.joints[:, :22].numpy() - joints_scene).max())
    print(f'restatement vs reference: rotation matrices {err_mat:.3e}, rotation vectors ({int(m.sum())} of {m.size} in range) '
          f'{err_vec:.3e}, translations {err_tr:.3e}, scene vertices {err_v:.3e}, scene joints {err_j:.3e}')
    print('rotation angles: min {:.3f} max {:.3f}'.format(*(lambda a: (a.min(), a.max()))(np.linalg.norm(ref_rv, axis=-1))))
    save = {'repr': rep, 'transf': transf, 'num_verts': np.int64(NUM_VERTS), 'vert_index': np.arange(0, NUM_VERTS, VERT_STEP),
            'cano_global_orient': go, 'cano_body_pose': bp, 'cano_joints': joints,
            'scene_global_orient': go_scene, 'scene_transl': tr_scene,
            'scene_verts': verts_scene[:, ::VERT_STEP].astype(np.float32), 'scene_joints': joints_scene.astype(np.float32),
            'measured_ref_error_rotmat': np.float64(err_mat), 'measured_ref_error_rotvec': np.float64(err_vec),
            'measured_ref_error_transl': np.float64(err_tr), 'measured_ref_error_verts': np.float64(max(err_v, err_j)),
            'measured_ref_error': np.array([err_mat, err_vec, err_tr, max(err_v, err_j)])}
    path = os.path.join(GOLD, 'export.npz')
    np.savez_compressed(path, **save)
    print(path, os.path.getsize(path))


if __name__ == '__main__':
    main()
