"""CPU: the float64 restatement of the export step (tests/export_ref.py) against the reference's own functions
(tests/golden/export.npz, scripts/make_golden_export.py), its properties at the hard rotations, and the round trip through the
clips the reference's loader made of the synthetic trees (tests/golden/video_loader.npz).

The reference computes its axis-angles and its body model in float32, so the restatement differs from it by the reference's own
rounding: the generator measured that difference (`measured_ref_error_*` in the fixture); the bars are 4 x those values, the
factor the optimiser parity tests use."""
import json
import os

import numpy as np
import pytest
import torch

import export_ref as ER
from helpers import golden
from oracle import geometry as G
from rohm_amd.utils import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR = 4
FLOAT32_SCALE = 1e-5          # sanity on the recorded figures: a few ulp of metre-sized float32 values, not a tolerance


@pytest.fixture(scope='module')
def fixture():
    g = golden('export.npz')
    tensors = synth.synthetic_smplx_tensors(0, num_verts=int(g['num_verts']))
    rep, transf = g['repr'], g['transf']
    C, T = rep.shape[:2]
    fc, ft = np.repeat(np.arange(C), T), np.tile(np.arange(T), C)
    pelvis = ER.fold_pelvis(tensors)
    cano, contact = ER.export_params(rep, fc, ft, pelvis)
    scene, _ = ER.export_params(rep, fc, ft, pelvis, transf=transf)
    return g, tensors, cano, scene, contact


def test_recorded_errors_are_float32_rounding(fixture):
    g = fixture[0]
    for k in ('rotmat', 'rotvec', 'transl', 'verts'):
        v = float(g['measured_ref_error_' + k])
        assert 0 < v < FLOAT32_SCALE, (k, v)
    assert np.array_equal(g['measured_ref_error'], [float(g['measured_ref_error_' + k]) for k in ('rotmat', 'rotvec', 'transl', 'verts')])


def test_canonical_rotations_match_the_reference(fixture):
    g, _, cano, _, contact = fixture
    n = len(cano)
    ref = np.concatenate([g['cano_global_orient'].reshape(n, 1, 3), g['cano_body_pose'].reshape(n, 21, 3)], axis=1).astype(np.float64)
    got = np.concatenate([cano[:, 0:3].reshape(n, 1, 3), cano[:, 16:79].reshape(n, 21, 3)], axis=1)
    err = np.abs(ER.rodrigues(got) - ER.rodrigues(ref)).max()
    print('canonical rotation matrices', err)
    assert err <= FACTOR * float(g['measured_ref_error_rotmat'])
    m = ER.rot_component_mask(ref)
    assert m.sum() > 0.9 * m.size
    err = np.abs(got - ref)[m].max()
    print('canonical rotation vectors', err)
    assert err <= FACTOR * float(g['measured_ref_error_rotvec'])
    rows = g['repr'].reshape(n, 294)
    assert np.abs(cano[:, 3:6] - rows[:, 16:19]).max() < 1e-15          # no transform: (t + d) - d, the translation passes through
    assert np.array_equal(cano[:, 6:16], rows[:, 280:290].astype(np.float64))
    assert np.array_equal(contact, rows[:, 290:294])


def test_scene_parameters_match_update_globalRT(fixture):
    g, _, _, scene, _ = fixture
    n = len(scene)
    ref = np.concatenate([g['scene_global_orient'].reshape(n, 1, 3), g['cano_body_pose'].reshape(n, 21, 3)], axis=1).astype(np.float64)
    got = np.concatenate([scene[:, 0:3].reshape(n, 1, 3), scene[:, 16:79].reshape(n, 21, 3)], axis=1)
    err = np.abs(ER.rodrigues(got) - ER.rodrigues(ref)).max()
    print('scene rotation matrices', err)
    assert err <= FACTOR * float(g['measured_ref_error_rotmat'])
    m = ER.rot_component_mask(ref)
    err = np.abs(got - ref)[m].max()
    print('scene rotation vectors', err)
    assert err <= FACTOR * float(g['measured_ref_error_rotvec'])
    err = np.abs(scene[:, 3:6] - g['scene_transl']).max()
    print('scene translations', err)
    assert err <= FACTOR * float(g['measured_ref_error_transl'])


def test_scene_vertices_match_points_coord_trans(fixture):
    """Skinning the exported scene-frame parameters gives the reference's canonical vertices taken to the scene."""
    g, tensors, _, scene, _ = fixture
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    out = G.BodyModel(tensors, dtype=torch.float64)(betas=t64(scene[:, 6:16]), global_orient=t64(scene[:, 0:3]),
                                                    body_pose=t64(scene[:, 16:79]), transl=t64(scene[:, 3:6]))
    bar = FACTOR * float(g['measured_ref_error_verts'])
    err = np.abs(out.vertices.numpy()[:, g['vert_index']] - g['scene_verts']).max()
    print('scene vertices', err)
    assert err <= bar
    err = np.abs(out.joints[:, :22].numpy() - g['scene_joints']).max()
    print('scene joints', err)
    assert err <= bar


def test_hard_rotations():
    rows, axis = ER.hard_rotations()
    R = ER.rot6d_to_rotmat(rows.astype(np.float32))
    assert np.abs(R @ np.swapaxes(R, -1, -2) - np.eye(3)).max() < 1e-14 and np.allclose(np.linalg.det(R), 1.0, atol=1e-14)
    rv = ER.rotmat_to_rotvec(R)
    assert np.array_equal(rv[0], np.zeros(3))
    assert np.abs(rv[1] - axis * 1e-7).max() < 1e-13              # float32 inputs: 1e-7 x 6e-8; not kornia's 2 v
    assert abs(np.linalg.norm(rv[2]) - (np.pi - 1e-4)) < 1e-6 and np.linalg.norm(rv[2]) <= np.pi
    assert np.abs(ER.rodrigues(rv) - R).max() < 1e-12
    assert np.abs(rv[3] - np.array([0.3, -0.8, 0.5])).max() < 1e-6           # Gram-Schmidt removes the scale and the shear
    # the shortest vector: a rotation by more than pi comes back with |aa| <= pi
    big = ER.rotmat_to_rotvec(ER.rodrigues(axis * 4.0))
    assert np.linalg.norm(big) <= np.pi and np.abs(ER.rodrigues(big) - ER.rodrigues(axis * 4.0)).max() < 1e-12


def test_out_of_range_index_gives_a_nan_row(fixture):
    g, tensors = fixture[0], fixture[1]
    rep, transf = g['repr'], g['transf']
    pelvis = ER.fold_pelvis(tensors)
    fc, ft = np.array([0, 3, 1, -1, 2]), np.array([0, 2, 7, 0, 6])
    got, contact = ER.export_params(rep, fc, ft, pelvis, transf=transf)
    assert np.isnan(got[[1, 2, 3]]).all() and np.isnan(contact[[1, 2, 3]]).all()
    assert np.isfinite(got[[0, 4]]).all()
    assert np.array_equal(got[4], fixture[3][2 * 7 + 6])


def test_rigid_after_inverse_is_a_change_of_frame(fixture):
    """frame='camera': with rigid = inv(cam2world) the exported body is the scene body seen from the camera."""
    g, tensors, _, scene, _ = fixture
    rep, transf = g['repr'], g['transf']
    C, T = rep.shape[:2]
    fc, ft = np.repeat(np.arange(C), T), np.tile(np.arange(T), C)
    cam2world = np.eye(4)
    cam2world[:3, :3] = ER.rodrigues(np.array([0.2, -0.4, 0.1]))
    cam2world[:3, 3] = [0.3, -1.2, 2.0]
    inv = np.linalg.inv(cam2world)
    cam, _ = ER.export_params(rep, fc, ft, ER.fold_pelvis(tensors), transf=transf, rigid=inv)
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    body = G.BodyModel(tensors, dtype=torch.float64)
    js = body(betas=t64(scene[:, 6:16]), global_orient=t64(scene[:, 0:3]), body_pose=t64(scene[:, 16:79]), transl=t64(scene[:, 3:6]),
              return_verts=False).joints[:, :22].numpy()
    jc = body(betas=t64(cam[:, 6:16]), global_orient=t64(cam[:, 0:3]), body_pose=t64(cam[:, 16:79]), transl=t64(cam[:, 3:6]),
              return_verts=False).joints[:, :22].numpy()
    # float64 throughout, except that the folded pelvis is a float32 number: 6e-8 x 1 m x |A_R - I|
    assert np.abs(jc - (js @ inv[:3, :3].T + inv[:3, 3])).max() < 5e-7


def test_round_trip_through_the_reference_loaders_clips():
    """Tree -> (reference loader, fixture) -> clips -> restatement -> world-frame parameters of the tree.  The figures are the
    distance the float32 representation puts between the two; they are recorded as `roundtrip_cpu_error` in
    profiles/export_parity.json, and 4 x that is the bar of the device round trip (tests/test_gpu_export.py)."""
    from rohm_amd.export import plan_frames
    r = ER.roundtrip_cpu(golden('video_loader.npz'), synth.synthetic_smplx_tensors(0), plan_frames)
    print('round trip', r)
    for dataset in ('prox', 'egobody'):
        rot, tr, betas = r[dataset]
        assert rot < FLOAT32_SCALE and tr < FLOAT32_SCALE and betas < 1e-6, (dataset, r[dataset])
    path = os.path.join(ROOT, 'profiles', 'export_parity.json')
    with open(path) as f:
        recorded = json.load(f)
    # the committed figure is this computation's (libm and BLAS may move the last digits)
    assert abs(recorded['roundtrip_cpu_error'] - r['roundtrip_cpu_error']) <= 0.25 * r['roundtrip_cpu_error']
