"""CPU: the numpy restatements of the clip-side loader work (tests/clips_ref.py) against what the reference's own functions
computed (tests/golden/clips.npz, tests/golden/video_loader.npz; scripts/make_golden_clips.py), and the host readers of
rohm_amd/data_loaders/dataloader_video.py on a tree rebuilt from the fixture."""
import warnings

import numpy as np
import pytest

import clips_ref as CR
import video_tree as VT
from helpers import golden
from oracle import rederive as RD
from rohm_amd.utils import synth

CASES = [(up, floor) for up in ('z', 'y') for floor in ('min', 'preset')]


@pytest.mark.parametrize('up_axis,floor', CASES)
def test_canonicalisation_and_representation_match_reference(up_axis, floor):
    g = golden('clips.npz')
    p = f'{up_axis}_{floor}_'
    N, L, ov = int(g['N']), int(g['L']), int(g['overlap'])
    jw, world = synth.synthetic_recording(int(g['seed']), N, up_axis)
    preset = float(g[p + 'preset']) if floor == 'preset' else None
    if preset is not None:
        assert preset == CR.clip_preset(jw, up_axis)
    out = CR.build_clips(jw, world, L, ov, up_axis, preset)
    assert out['starts'].tolist() == [0, 14, 28]
    for k in ('cano_joints', 'global_orient', 'transl', 'transf_matrix'):
        np.testing.assert_allclose(out[k], g[p + k], rtol=0, atol=1e-9, err_msg=k)
    # the oracle's get_repr_smplx on the reference's own canonical clip: bit-exact, as tests/test_rederive_oracle.py holds it
    for c, s in enumerate(out['starts']):
        prm = dict(CR.split_world(world[s:s + L]), global_orient=g[p + 'global_orient'][c], transl=g[p + 'transl'][c])
        full = RD.full_repr(RD.get_repr_smplx(g[p + 'cano_joints'][c], prm))
        np.testing.assert_array_equal(full, g[p + 'repr'][c])
    # ... and end to end from the restated canonicalisation (its 1e-16 differences move no float32 rounding here)
    np.testing.assert_allclose(out['repr'], g[p + 'repr'], rtol=0, atol=1e-9)
    # the synthetic recording does what it is for
    fc = g[p + 'repr'][..., 290:]
    assert (fc.mean(axis=(0, 1)) > 0.1).all() and (fc.mean(axis=(0, 1)) < 0.9).all()
    assert CR.contact_margin(g[p + 'cano_joints']) > 1e-3 and not np.isnan(g[p + 'repr']).any()


def test_preset_floor_zero_counts_as_not_given():
    jw, world = synth.synthetic_recording(3, 16, 'z')
    a, b = CR.build_clips(jw, world, 16, preset_floor_height=0.0), CR.build_clips(jw, world, 16)
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_degenerate_clip_matches_reference_nan_pattern():
    g = golden('clips.npz')
    L = int(g['L'])
    jw, world = synth.synthetic_recording(int(g['seed']), L, 'z', degenerate_frames=CR.DEGENERATE_FRAMES)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        out = CR.build_clips(jw, world, L)
    ref = g['degenerate_repr']
    nan = np.isnan(ref)[0]
    # frame 5 is patched with frame 4; frame 9 stays NaN
    assert sorted(set(np.argwhere(nan)[:, 0].tolist())) == [8, 9]
    assert nan[9, 0] and nan[8, 1] and nan[9, 1] and nan[8, 4:6].all() and nan[9, 22:154].all() and not nan[:, 154:].any()
    assert np.array_equal(np.isnan(out['repr']), np.isnan(ref))
    np.testing.assert_allclose(np.nan_to_num(out['repr']), np.nan_to_num(ref), rtol=0, atol=1e-9)


def test_local_factor_measurement():
    """The figure behind tests/test_gpu_clips.py::LOCAL_FACTOR: how far the reference's float32 quaternion flow is from
    the same computation in float64, on local_positions / local_vel, in units of the facing-conditioning term times
    the vector length -- re-measured on the fixture's cases (the GPU test's other inputs gave smaller figures)."""
    worst = 0.0
    for up_axis in ('z', 'y'):
        jw, world = synth.synthetic_recording(CR.CLIP_SEED, CR.CLIP_N, up_axis)
        a = CR.build_clips(jw, world, CR.CLIP_L, CR.CLIP_OVERLAP, up_axis)
        b = CR.build_clips(jw, world, CR.CLIP_L, CR.CLIP_OVERLAP, up_axis, all_f64=True)
        std = synth.synthetic_stats(3)[1]
        worst = max(worst, CR.local_ratio(a['repr'], b['repr'], a['cano_joints']),
                    CR.local_ratio(a['repr'], b['repr'], a['cano_joints'], std))
    assert 0.0 < worst <= 0.0112


def test_undistort_then_distort_returns_the_input():
    """Five fixed-point iterations at PROX-like coefficients leave a residual of 6.7e-8 px (float64, measured over a
    97 x 55 grid covering the 1920 x 1080 image; 1.5e-9 px after six, 1e-12 px after eight); the bound is 4x that."""
    xs, ys = np.meshgrid(np.linspace(0, 1919, 97), np.linspace(0, 1079, 55))
    p = np.stack([xs, ys], -1)
    u = CR.undistort_pixels(p, CR.PROX_K, CR.PROX_DIST)
    assert np.abs(u - p).max() > 5.0                                    # the lens model does something
    assert np.abs(CR.distort_pixels(u, CR.PROX_K, CR.PROX_DIST) - p).max() <= 4 * 6.7e-8
    # without distortion the undistortion is the identity; the mirrored variant keeps the confidence
    assert np.abs(CR.undistort_pixels(p, CR.PROX_K, np.zeros(5)) - p).max() < 1e-9
    kp = np.concatenate([p, np.full(p.shape[:-1] + (1,), 0.7)], -1)
    out = CR.undistort_keypoints(kp, CR.PROX_K, CR.PROX_DIST)
    assert np.array_equal(out[..., 2], kp[..., 2])
    mirrored = CR.undistort_pixels(np.stack([1919 - xs, ys], -1), CR.PROX_K, CR.PROX_DIST)
    np.testing.assert_allclose(out[..., 0], 1919 - mirrored[..., 0], atol=1e-12)
    np.testing.assert_allclose(out[..., 1], mirrored[..., 1], atol=1e-12)


def test_mask_rule_on_hand_made_cases():
    kp = np.zeros((4, 22, 3))
    kp[..., 2] = 0.9
    mask = np.ones((4, 25))
    kp[1, 7, 2] = 0.1          # left ankle not detected
    mask[2, 11] = 0.0          # right foot occluded in depth
    kp[3, 3, 2] = 0.2          # exactly at the threshold: not visible
    jv, vv = CR.visibility_masks(kp, mask)
    assert jv.shape == (4, 22) and vv.shape == (4, 294)
    assert jv[0].all() and vv[0].all()
    assert jv[1].sum() == 21 and jv[1, 7] == 0
    assert vv[1, :22].all() and vv[1, 280:290].all()
    hidden = lambda j: [22 + 3 * j + k for k in range(3)] + [88 + 3 * j + k for k in range(3)] + \
        [154 + 6 * (j - 1) + k for k in range(6)]
    off = np.flatnonzero(vv[1] == 0).tolist()
    assert off == sorted(hidden(7) + [290, 291])                       # joint 7's channels and the left-foot contacts
    off = np.flatnonzero(vv[2] == 0).tolist()
    assert off == sorted(hidden(11) + [292, 293])
    assert np.flatnonzero(vv[3] == 0).tolist() == sorted(hidden(3))
    # joint 0 has no body_pose_6d channels
    kp[0, 0, 2] = 0.0
    _, vv = CR.visibility_masks(kp, mask)
    assert np.flatnonzero(vv[0] == 0).tolist() == [22, 23, 24, 88, 89, 90]


@pytest.mark.parametrize('dataset', ['prox', 'egobody'])
def test_host_readers_on_a_tree_rebuilt_from_the_fixture(dataset, tmp_path):
    from rohm_amd.data_loaders import dataloader_video as DV
    g = golden('video_loader.npz')
    a = VT.tree_arrays_from_fixture(g, dataset)
    paths = VT.write_tree(str(tmp_path), dataset, a)
    rec_name = str(a['recording_name'])
    read = DV.read_prox_recording if dataset == 'prox' else DV.read_egobody_recording
    rec = read(paths['init_root'], paths['base_dir'], rec_name)
    n = VT.N_FRAMES
    assert rec['frame_names'] == [str(s) for s in a['frame_names']] and rec['scene_name'] == str(a['scene_name'])
    for k, (lo, hi) in VT.PARAM_SLICES.items():
        assert rec['params'][k].dtype == np.float32 and np.array_equal(rec['params'][k], a['params'][:, lo:hi])
    person = 0 if dataset == 'prox' else int(a['target_idx'])
    want = a['keypoints'][:, person][:, DV.OPENPOSE_TO_SMPL[:22]].astype(np.float64)
    want[VT.EMPTY_FRAME] = 0.0
    assert rec['keypoints'].shape == (n, 22, 3) and rec['keypoints'].dtype == np.float64     # one frame without people
    assert np.array_equal(rec['keypoints'], want)
    assert np.array_equal(rec['mask_joint'], a['mask_joint'])
    assert rec['color_cam']['k'] == a['cam_k'].tolist() and rec['color_cam']['f'] == a['cam_f'].tolist()
    if dataset == 'prox':
        assert np.array_equal(rec['cam2world'], a['cam2world'])
    else:
        assert (rec['view'], rec['body_idx'], rec['gender_gt']) == ('sub_1', 1, 'female')
        assert rec['fitting_gt_root'].endswith(f'smplx_interactee_val/{rec_name}/body_idx_1')
        assert np.array_equal(rec['master2world'], a['master2world'])
        assert np.array_equal(rec['cam2world'], a['master2world'] @ a['sub2main'])
        assert np.array_equal(rec['params_gt']['body_pose'], a['params_gt'][:, 16:79])
        with pytest.raises(KeyError):
            DV.read_egobody_info(paths['base_dir'], 'recording_unknown')
    mean_dict, std_dict, mean, std = DV.read_stats(paths['logdir'])
    assert list(mean_dict) == DV.REPR_LIST and np.array_equal(mean, a['mean']) and np.array_equal(std, a['std'])
    assert sum(DV.REPR_DIM_DICT.values()) == 294


@pytest.mark.parametrize('dataset', ['prox', 'egobody'])
def test_restatement_reproduces_the_reference_loader_items(dataset):
    """The reference's own DataloaderVideo items (fixture) from the restatements alone: oracle frames_to_world +
    clips_ref.build_clips + the mask rule (+ the undistortion, which the fixture does not pin: it was recorded with this
    restatement standing in for cv2.undistortPoints)."""
    from oracle import frames as OF
    from oracle import geometry as G
    g = golden('video_loader.npz')
    a = VT.tree_arrays_from_fixture(g, dataset)
    params = {k: a['params'][:, lo:hi] for k, (lo, hi) in VT.PARAM_SLICES.items()}
    cam2world = a['cam2world'] if dataset == 'prox' else a['master2world'] @ a['sub2main']
    body = G.BodyModel(synth.synthetic_smplx_tensors(0))
    jw, world = OF.frames_to_world(body, params, cam2world.astype(np.float32))
    up_axis = 'z' if dataset == 'prox' else 'y'
    for floor in ('min', 'floor'):
        p = f'{dataset}_pose_{floor}_'
        assert int(g[p + 'len']) == 3
        preset = float(g[f'{dataset}_floor_height']) if floor == 'floor' else None
        out = CR.build_clips(jw, world, VT.CLIP_LEN, VT.OVERLAP, up_axis, preset, stats=(a['mean'], a['std']))
        assert CR.contact_margin(out['cano_joints']) > 1e-3
        for i in range(3):
            q = f'{p}item{i}_'
            np.testing.assert_allclose(out['cano_joints'][i], g[q + 'noisy_joints'], atol=1e-6)
            np.testing.assert_allclose(out['transf_matrix'][i], g[q + 'transf_matrix'], atol=1e-6)
            np.testing.assert_allclose(out['repr'][i], g[q + 'motion_repr_noisy'], atol=2e-6)
            np.testing.assert_array_equal(out['repr'][i][:, 290:].astype(np.float32), g[q + 'motion_repr_noisy'][:, 290:])
    person = 0 if dataset == 'prox' else int(a['target_idx'])
    kp = a['keypoints'][:, person][:, [8, 12, 9, 8, 13, 10, 8, 14, 11, 1, 20, 23, 1, 5, 2, 0, 5, 2, 6, 3, 7, 4]].astype(np.float64)
    kp[VT.EMPTY_FRAME] = 0.0
    jv, vv = CR.visibility_masks(kp, a['mask_joint'])
    for i, s in enumerate((0, 6, 12)):
        q = f'{dataset}_pose_min_item{i}_'
        assert np.array_equal(jv[s:s + 8], g[q + 'mask_joint_vis']) and np.array_equal(vv[s:s + 8], g[q + 'mask_vec_vis'])
        want = CR.undistort_keypoints(kp[s:s + 8], a['cam_mtx'], a['cam_k']) if dataset == 'prox' else kp[s:s + 8]
        np.testing.assert_allclose(want, g[q + 'keypoints_2d'], atol=1e-3)      # the reference flips x in float32 for PROX
