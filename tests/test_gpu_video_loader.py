"""GPU: the native DataloaderVideo (rohm_amd/data_loaders/dataloader_video.py) on PROX / EgoBody trees rebuilt from
tests/golden/video_loader.npz, against every item the reference's own DataloaderVideo produced on those trees
(scripts/make_golden_clips.py), and its batches fed into the PROX iteration loop.

The fixture's PROX `keypoints_2d` were recorded with the test restatement standing in for cv2.undistortPoints (cv2 is
absent where fixtures are made): they pin the flips, the shapes and the dtype, not the undistortion arithmetic."""
import types

import numpy as np
import pytest
import torch

import clips_ref as CR
import video_tree as VT
from helpers import golden
from rohm_amd.utils import synth

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GEOM_TOL, KP_TOL = 5e-6, 1e-3                       # as tests/test_gpu_clips.py
LOCAL_FACTOR = 4 * 0.0112                           # tests/test_gpu_clips.py::_close
ITEM_KEYS = {'motion_repr_noisy', 'noisy_joints', 'noisy_joints_scene_coord', 'transf_matrix', 'cano_smplx_params_dict',
             'frame_name', 'focal_length', 'camera_center', 'keypoints_2d', 'mask_joint_vis', 'mask_vec_vis'}


def _layer():
    from rohm_amd.body_model import SMPLXLayer
    return SMPLXLayer.from_tensors(synth.synthetic_smplx_tensors(0)).to(DEV)


@pytest.fixture(scope='module')
def trees(tmp_path_factory):
    g = golden('video_loader.npz')
    out = {}
    for dataset in ('prox', 'egobody'):
        a = VT.tree_arrays_from_fixture(g, dataset)
        out[dataset] = (a, VT.write_tree(str(tmp_path_factory.mktemp(dataset)), dataset, a))
    return g, out


def _loader(trees, dataset, task, use_floor=False, **kw):
    from rohm_amd.data_loaders.dataloader_video import DataloaderVideo
    g, t = trees
    a, paths = t[dataset]
    return DataloaderVideo(dataset=dataset, init_root=paths['init_root'], base_dir=paths['base_dir'], body_model_path=_layer(),
                           recording_name=str(a['recording_name']), use_scene_floor_height=use_floor,
                           repr_abs_only=(task == 'traj'), task=task, overlap_len=VT.OVERLAP, clip_len=VT.CLIP_LEN,
                           logdir=paths['logdir'], device=DEV,
                           floor_heights={str(a['scene_name']): float(g[f'{dataset}_floor_height'])}, **kw)


@pytest.mark.parametrize('use_floor', [False, True])
@pytest.mark.parametrize('task', ['pose', 'traj'])
@pytest.mark.parametrize('dataset', ['prox', 'egobody'])
def test_items_match_the_reference_loader(trees, dataset, task, use_floor):
    g = trees[0]
    ds = _loader(trees, dataset, task, use_floor)
    p = f"{dataset}_{task}_{'floor' if use_floor else 'min'}_"
    assert len(ds) == int(g[p + 'len']) == 3
    for attr in ('body_feat_dim', 'traj_feat_dim', 'pose_feat_dim', 'n_samples', 'clip_len'):
        assert getattr(ds, attr) == int(g[p + attr]), attr
    assert ds.scene_floor_height == float(g[p + 'scene_floor_height'])
    assert ds.Mean.shape == ds.Std.shape == (294,) and list(ds.Mean_dict) == list(ds.Std_dict) and len(ds.Mean_dict) == 14
    assert ds.color_cam['f'] == trees[1][dataset][0]['cam_f'].tolist()
    std = ds.Std
    keys = set(ITEM_KEYS) | ({'gt_joints_scene_coord'} if dataset == 'egobody' else set()) | \
        ({'cond', 'control_cond'} if task == 'traj' else set())
    for i in range(len(ds)):
        item = ds[i]
        assert set(item) == keys
        q = f'{p}item{i}_'
        ref = {k: g[q + k] for k in keys - {'cano_smplx_params_dict', 'frame_name'}}
        for k, r in ref.items():
            assert item[k].shape == r.shape and item[k].dtype == r.dtype, (k, item[k].dtype, r.dtype)
        assert item['frame_name'] == [str(s) for s in g[q + 'frame_name']] == ds.frame_name_list[i]
        cano = ref['noisy_joints'][None].astype(np.float64)
        assert CR.contact_margin(cano) > 1e-3
        for k in ('noisy_joints', 'noisy_joints_scene_coord', 'transf_matrix', 'focal_length', 'camera_center') + \
                (('gt_joints_scene_coord',) if dataset == 'egobody' else ()):
            assert np.abs(item[k] - ref[k]).max() <= GEOM_TOL, k
        for k in ('global_orient', 'transl', 'betas', 'body_pose'):
            r = g[f'{q}params_{k}']
            v = item['cano_smplx_params_dict'][k]
            assert v.shape == r.shape and v.dtype == r.dtype == np.float32 and np.abs(v - r).max() <= GEOM_TOL, k
        lim = CR.repr_limits(ref['motion_repr_noisy'][None], cano, std, 2e-5, LOCAL_FACTOR)[0]
        err = np.abs(item['motion_repr_noisy'].astype(np.float64) - ref['motion_repr_noisy'])
        assert (err <= lim).all(), (err.max(), np.argwhere(err > lim)[:5].tolist())
        assert np.array_equal(item['motion_repr_noisy'][:, 290:], ref['motion_repr_noisy'][:, 290:])
        assert np.array_equal(item['mask_joint_vis'], ref['mask_joint_vis'])
        assert np.array_equal(item['mask_vec_vis'], ref['mask_vec_vis'])
        assert np.abs(item['keypoints_2d'][..., :2] - ref['keypoints_2d'][..., :2]).max() <= KP_TOL
        assert np.array_equal(item['keypoints_2d'][..., 2], ref['keypoints_2d'][..., 2])
        if task == 'traj':
            assert np.array_equal(item['cond'], item['motion_repr_noisy'][:, [0, 2, 3, 6, 7, 8, 9, 10, 11, 12, 16, 17, 18]])
            assert np.array_equal(item['control_cond'], item['motion_repr_noisy'][:, -272:])
            assert np.abs(item['cond'] - ref['cond']).max() <= lim[:, :22].max()


@pytest.mark.parametrize('dataset', ['prox', 'egobody'])
def test_batches_on_the_device_and_items_in_a_dataloader(trees, dataset):
    ds = _loader(trees, dataset, 'traj')
    got = list(ds.batches(2))
    assert [b['motion_repr_noisy'].shape[0] for b in got] == [2, 1]
    want = {'motion_repr_noisy': (7, 294), 'noisy_joints': (8, 22, 3), 'noisy_joints_scene_coord': (8, 22, 3),
            'transf_matrix': (4, 4), 'focal_length': (2,), 'camera_center': (2,), 'keypoints_2d': (8, 22, 3),
            'mask_joint_vis': (8, 22), 'mask_vec_vis': (8, 294), 'cond': (7, 13), 'control_cond': (7, 272)}
    if dataset == 'egobody':
        want['gt_joints_scene_coord'] = (8, 22, 3)
    for b in got:
        assert set(b) == set(want) | {'cano_smplx_params_dict', 'frame_name'}
        n = b['cond'].shape[0]
        for k, s in want.items():
            assert b[k].is_cuda and b[k].dtype == torch.float32 and tuple(b[k].shape) == (n,) + s, k
        assert {k: tuple(v.shape[1:]) for k, v in b['cano_smplx_params_dict'].items()} == \
            {'global_orient': (8, 3), 'transl': (8, 3), 'betas': (8, 10), 'body_pose': (8, 63)}
        assert all(v.is_cuda for v in b['cano_smplx_params_dict'].values())
        assert b['frame_name'].shape == (n, 8)
    # the host items collate to the same batches, without the GPU
    dl = torch.utils.data.DataLoader(ds, batch_size=2, shuffle=False)
    for b, hb in zip(got, dl):
        for k in want:
            assert torch.equal(b[k].cpu(), hb[k].float()) or k == 'keypoints_2d', k
        assert np.array_equal(np.asarray(hb['frame_name']).T, b['frame_name'])
        assert torch.equal(b['cano_smplx_params_dict']['transl'].cpu(), hb['cano_smplx_params_dict']['transl'])
    # what a spawned worker would receive carries no device state and still serves the items
    import pickle
    clone = pickle.loads(pickle.dumps(ds))
    assert not hasattr(clone, '_device_data') and not hasattr(clone, 'smplx_neutral')
    assert np.array_equal(clone[2]['motion_repr_noisy'], ds[2]['motion_repr_noisy'])


class _Stub:
    def __init__(self, outputs):
        self.outputs = list(outputs)

    def eval_losses(self, model=None, batch=None, shape=None, **kw):
        out = self.outputs.pop(0)
        assert list(out.shape) == list(shape), (out.shape, shape)
        return None, out


def test_batches_feed_the_prox_iterations(trees):
    """`batches(2)` of the traj- and the pose-task loader into `run_prox_iterations` with stub stages (cf.
    tests/test_gpu_scheme.py::test_prox_glue_with_stub_stages), sample_iter 2."""
    from rohm_amd import inference as INF
    traj_ds, pose_ds = _loader(trees, 'prox', 'traj'), _loader(trees, 'prox', 'pose')
    args = types.SimpleNamespace(sample_iter=2, repr_abs_only=True, iter2_cond_noisy_traj=True, iter2_cond_noisy_pose=True,
                                 early_stop=False, cond_fn_with_grad=False, timestep_respacing_eval='')
    L = VT.CLIP_LEN
    body_t = synth.synthetic_smplx_tensors(0)
    stats = (traj_ds.Mean.astype(np.float32), traj_ds.Std.astype(np.float32))
    seen = 0
    for bt, bp in zip(traj_ds.batches(2), pose_ds.batches(2)):
        B = bt['cond'].shape[0]
        traj_out = [synth.walking_motion(160 + i, B, L - 1, *stats, body_t)[:, :, list(INF.ABS_TRAJ_CH)].contiguous().to(DEV)
                    for i in range(2)]
        pose_out = [synth.walking_motion(170 + i, B, L - 2, *stats, body_t).permute(0, 2, 1).unsqueeze(2).contiguous().to(DEV)
                    for i in range(2)]
        diffs = {'trajnet': _Stub(traj_out[:1]), 'trajnet_control': _Stub(traj_out[1:]), 'posenet': _Stub(pose_out)}
        pose, traj, recs = INF.run_prox_iterations(args, {'trajnet': None, 'trajnet_control': None, 'posenet': None}, diffs,
                                                   bt, bp, traj_ds, pose_ds, _layer())
        assert len(recs) == 2 and all(tuple(r.shape) == (B, L - 2, 22) for r in recs)
        assert all(torch.isfinite(r).all() for r in recs)
        assert tuple(pose.shape) == (B, 294, 1, L - 2) and tuple(traj.shape) == (B, L - 1, 13)
        assert tuple(bp['cond'].shape) == (B, 294, 1, L - 2)
        seen += B
    assert seen == 3


def test_loader_errors(trees):
    from rohm_amd._lib import RohmHipError
    from rohm_amd.data_loaders.dataloader_video import DataloaderVideo
    a, paths = trees[1]['prox']
    kw = dict(dataset='prox', init_root=paths['init_root'], base_dir=paths['base_dir'], body_model_path=_layer(),
              recording_name=str(a['recording_name']), clip_len=8, logdir=paths['logdir'])
    with pytest.raises(RohmHipError):
        DataloaderVideo(device='cpu', **kw)
    with pytest.raises(ValueError):
        DataloaderVideo(device=DEV, use_scene_floor_height=True, **kw)          # no floor table given
    with pytest.raises(ValueError):
        DataloaderVideo(device=DEV, task='both', **kw)
    assert len(DataloaderVideo(device=DEV, **dict(kw, clip_len=30))) == 0       # 20 frames: no clip
