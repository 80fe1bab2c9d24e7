"""GPU: reconstructing a generic track -- `rohm_track_resample` (csrc/track.hip) against its float64 restatement
(tests/track_ref.py, whose slerp tests/test_track_ref.py holds against scipy), `DataloaderTrack` pinned to `DataloaderVideo`
on the video loader's fixture trees, the tail window, gaps in the visibility masks, the `track` driver end to end and the way
back through `export.resample_params`.

Kernel and restatement are both float64 on the same inputs and differ by libm and fma contraction only.  Bars: rotations
geodesic <= 1e-12 rad; transl / betas <= 1e-13 max(1, |v|); keypoint x / y within one float32 ulp; confidences, masks, gap,
src_index equal.  All rotation inputs stay below 3.0 rad with at most 2.0 rad between bracketing frames, where the
restatement is held to scipy.  The measured maxima go to profiles/track_parity.json."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

import track_ref as TR
import video_tree as VT
from helpers import golden
from rohm_amd.utils import synth

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROT_BAR, LIN_BAR = 1e-12, 1e-13
PARITY = {}


def _record(key, value):
    path = os.path.join(ROOT, 'profiles', 'track_parity.json')
    PARITY[key] = max(float(value), PARITY.get(key, 0.0))
    try:
        with open(path) as f:
            data = json.load(f)
    except (OSError, ValueError):
        data = {}
    data.setdefault('gpu', {}).update(PARITY)
    try:
        with open(path, 'w') as f:
            json.dump(data, f, indent=1, sort_keys=True)
            f.write('\n')
    except OSError:
        pass


def _layer():
    from rohm_amd.body_model import SMPLXLayer
    return SMPLXLayer.from_tensors(synth.synthetic_smplx_tensors(0)).to(DEV)


def _host(d):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in d.items()}


def _compare(got, want, tag):
    """Every output of the kernel against the restatement, at the bars of the module docstring."""
    got = _host(got)
    assert np.array_equal(got['src_index'], want['src_index']) and got['src_index'].dtype == np.int32
    assert np.array_equal(got['gap'], want['gap']) and got['gap'].dtype == np.uint8
    p, q = got['params'], want['params']
    assert p.shape == q.shape and p.dtype == np.float64 and np.isfinite(p).all()
    rot = max(TR.geodesic(p[:, c:c + 3], q[:, c:c + 3]).max() for c in TR.ROT_COLS)
    lin = (np.abs(p[:, 3:16] - q[:, 3:16]) / np.maximum(1.0, np.abs(q[:, 3:16]))).max()
    print(f'{tag}: rotations max geodesic {rot:.3e} rad (bar {ROT_BAR:.0e}), transl / betas max relative {lin:.3e} (bar {LIN_BAR:.0e})')
    _record(tag + '_rotation_max_geodesic_rad', rot)
    _record(tag + '_transl_betas_max_rel', lin)
    assert rot <= ROT_BAR and lin <= LIN_BAR
    assert max(np.linalg.norm(p[:, c:c + 3], axis=-1).max() for c in TR.ROT_COLS) <= np.pi + 1e-12
    if want['keypoints'] is not None:
        k, r = got['keypoints'], want['keypoints']
        assert k.shape == r.shape and k.dtype == np.float32
        ulps = (np.abs(k[..., :2].astype(np.float64) - r[..., :2]) / np.spacing(np.abs(r[..., :2]))).max()
        print(f'{tag}: keypoint x / y max {ulps:.2f} float32 ulp (bar 1)')
        _record(tag + '_keypoint_xy_max_ulp', ulps)
        assert ulps <= 1.0
        assert np.array_equal(k[..., 2], r[..., 2])
    if want['mask_joint'] is not None:
        assert np.array_equal(got['mask_joint'], want['mask_joint']) and got['mask_joint'].dtype == np.float32


def _random_track(n, fps, seed, J=22, M=25):
    g = np.random.Generator(np.random.PCG64(seed))
    params = TR.smooth_params(g, n)
    kp = np.concatenate([g.uniform(size=(n, J, 2)) * np.array([1920.0, 1080.0]), g.uniform(0.05, 1.0, size=(n, J, 1))], -1).astype(np.float32)
    kp[g.uniform(size=(n, J)) < 0.15] = 0.0                               # detections the estimator missed: (0, 0, 0)
    mask = (g.uniform(size=(n, M)) > 0.3).astype(np.float32)
    return np.arange(n) / fps, params, kp, mask


# ---- (a) kernel against restatement ---------------------------------------------------------------------------------------
INVALID_37 = [0, 5, 10, 11, 20, 21, 22, 23, 24, 36]                       # runs of 1, 2 and 5; first and last frame


def test_kernel_matches_the_restatement():
    from rohm_amd.data_loaders.track import default_max_gap, plan_times, resample_track
    ts, params, kp, mask = _random_track(37, 25.0, 7)
    valid = np.ones(37, bool)
    valid[INVALID_37] = False
    params[~valid] = np.nan                                               # rows without a fit are never read
    td = plan_times(ts, valid)
    assert np.array_equal(td, TR.plan_times(ts, valid)) and len(td) == 41 and td[0] == ts[1]
    max_gap = default_max_gap(ts)
    assert abs(max_gap - 0.06) < 1e-12
    got = resample_track(ts, valid, params, kp, mask, td, None, DEV)
    want = TR.resample(ts, valid, params, kp, mask, td, max_gap)
    assert 0 < want['gap'].sum() < len(td) and (want['keypoints'][want['gap'] == 0, :, 2] == 0).any()
    _compare(got, want, 'kernel_25_to_30')
    again = resample_track(ts, valid, params, kp, mask, td, None, DEV)
    assert all(torch.equal(again[k], got[k]) for k in got)               # no atomics: the same input gives the same bits
    # holds before the first and after the last valid frame, a wide max_gap, device tensors in, no keypoints / masks
    td2 = np.concatenate([[-0.5, 0.0, ts[1]], td[3:30] + 0.003, [ts[35], 1.47, 9.0]])
    dev = lambda a, t: torch.from_numpy(np.ascontiguousarray(a)).to(DEV, t)      # noqa: E731
    got = resample_track(ts, valid, dev(np.nan_to_num(params), torch.float64), dev(kp[:, :3], torch.float32), None, td2, 0.5, DEV)
    want = TR.resample(ts, valid, params, kp[:, :3], None, td2, 0.5)
    assert want['gap'].tolist() == [1, 1] + [0] * 29 + [1, 1] and got['mask_joint'] is None
    _compare(got, want, 'kernel_holds')
    got = resample_track(ts, valid, np.nan_to_num(params), None, None, td, 0.0, DEV)
    _compare(got, TR.resample(ts, valid, params, None, None, td, 0.0), 'kernel_params_only')
    assert tuple(resample_track(ts, valid, np.nan_to_num(params), kp, mask, np.zeros(0), None, DEV)['params'].shape) == (0, 79)


def test_kernel_refuses_bad_arguments():
    from rohm_amd import _lib
    from rohm_amd.data_loaders.track import resample_track
    ts, params, kp, mask = _random_track(6, 25.0, 2)
    with pytest.raises(_lib.RohmHipError, match='no CPU fallback'):
        resample_track(ts, np.ones(6, bool), params, device='cpu')
    with pytest.raises(ValueError, match='strictly increasing'):
        resample_track(ts[::-1], np.ones(6, bool), params, device=DEV)
    with pytest.raises(ValueError, match='at least one valid'):
        resample_track(ts, np.zeros(6, bool), params, device=DEV)
    with pytest.raises(ValueError):
        resample_track(ts, np.ones(6, bool), params[:, :78], device=DEV)
    lib, stream = _lib.lib(), _lib.stream_ptr(torch.device(DEV))
    t = torch.from_numpy(ts).to(DEV)
    p = torch.from_numpy(params).to(DEV)
    o, si, gp = torch.empty(6, 79, device=DEV, dtype=torch.float64), torch.empty(6, device=DEV, dtype=torch.int32), \
        torch.empty(6, device=DEV, dtype=torch.uint8)

    def call(vi, n=6, nv=None, J=0, max_gap=0.06):
        v = torch.tensor(vi, device=DEV, dtype=torch.int32)
        return lib.rohm_track_resample(t.data_ptr(), v.data_ptr(), p.data_ptr(), None, None, t.data_ptr(), max_gap, n, len(vi) if nv is None
                                       else nv, J, 0, 6, o.data_ptr(), None, None, si.data_ptr(), gp.data_ptr(), stream)
    assert call([0, 1, 2, 3, 4, 5]) == 0
    assert call([0], nv=0) == -1 and b'Nv' in lib.rohm_last_error()
    assert call([0, 2, 1]) == -1 and b'ascending' in lib.rohm_last_error()
    assert call([0, 6]) == -1 and b'outside' in lib.rohm_last_error()
    assert call([-1, 3]) == -1 and b'outside' in lib.rohm_last_error()
    assert call([0, 1], J=2) == -1 and b'keypoints' in lib.rohm_last_error()
    assert call([0, 1], max_gap=float('nan')) == -1


# ---- (b) 60 fps -> 30 fps: bitwise the even source rows -------------------------------------------------------------------
def test_60_fps_is_copied_through():
    from rohm_amd.data_loaders.track import resample_track
    ts, params, kp, mask = _random_track(41, 60.0, 9)
    got = _host(resample_track(ts, np.ones(41, bool), params, kp, mask, None, None, DEV))
    assert got['params'].shape == (21, 79) and got['src_index'].tolist() == list(range(0, 41, 2)) and not got['gap'].any()
    assert got['params'].tobytes() == params[::2].tobytes()
    assert got['keypoints'].tobytes() == kp[::2].tobytes() and got['mask_joint'].tobytes() == mask[::2].tobytes()


# ---- (c) pinned to the existing loader ------------------------------------------------------------------------------------
def track_from_tree(a, dataset, floor_height, n=None, fps=30.0):
    """The arrays of a `video_tree` recording as a track dict (camera-frame float32 fits, BODY_25 keypoints of the person the
    loader reads, zeros where nobody was detected)."""
    n = len(a['params']) if n is None else n
    person = 0 if dataset == 'prox' else int(a['target_idx'])
    kp = a['keypoints'][:n, person].astype(np.float32) * a['people_present'][:n, None, None]
    d = {k: a['params'][:n, lo:hi] for k, (lo, hi) in VT.PARAM_SLICES.items()}
    d.update(cam2world=a['cam2world'] if dataset == 'prox' else np.matmul(a['master2world'], a['sub2main']), fps=fps,
             keypoints_2d=kp.astype(np.float32), mask_joint=a['mask_joint'][:n], up_axis='z' if dataset == 'prox' else 'y',
             focal_length=a['cam_f'], camera_center=a['cam_c'], floor_height=floor_height, frame_names=a['frame_names'][:n],
             recording_name=str(a['recording_name']))
    if dataset == 'prox':
        d.update(camera_mtx=a['cam_mtx'], dist_coeffs=a['cam_k'])
    return d


@pytest.fixture(scope='module')
def trees(tmp_path_factory):
    g = golden('video_loader.npz')
    out = {}
    for dataset in ('prox', 'egobody'):
        a = VT.tree_arrays_from_fixture(g, dataset)
        root = tmp_path_factory.mktemp(dataset)
        path = str(root / 'track.npz')
        np.savez(path, **track_from_tree(a, dataset, float(g[f'{dataset}_floor_height'])))
        out[dataset] = (a, VT.write_tree(str(root), dataset, a), path)
    return g, out


@pytest.mark.parametrize('use_floor', [False, True])
@pytest.mark.parametrize('task', ['pose', 'traj'])
@pytest.mark.parametrize('dataset', ['prox', 'egobody'])
def test_a_30_fps_track_is_the_video_loader(trees, dataset, task, use_floor):
    from rohm_amd.data_loaders.dataloader_video import DataloaderVideo
    from rohm_amd.data_loaders.track import DataloaderTrack
    g, t = trees
    a, paths, track = t[dataset]
    layer = _layer()
    kw = dict(use_scene_floor_height=use_floor, repr_abs_only=(task == 'traj'), task=task, overlap_len=VT.OVERLAP, clip_len=VT.CLIP_LEN,
              logdir=paths['logdir'], device=DEV)
    ref = DataloaderVideo(dataset=dataset, init_root=paths['init_root'], base_dir=paths['base_dir'], body_model_path=layer,
                          recording_name=str(a['recording_name']),
                          floor_heights={str(a['scene_name']): float(g[f'{dataset}_floor_height'])}, **kw)
    ds = DataloaderTrack(track, body_model_path=layer, **kw)
    assert ds.dataset == 'track' and len(ds) == len(ref) == 3 and ds.clip_starts.tolist() == [0, 6, 12]
    keys = set(ref._device_data) - {'gt_joints_scene_coord'}
    assert set(ds._device_data) == keys
    for k in sorted(keys):
        assert torch.equal(ds._device_data[k], ref._device_data[k]), k
    assert ds.frame_name_list == ref.frame_name_list
    assert torch.equal(ds.cam_R, ref.cam_R) and torch.equal(ds.cam_t, ref.cam_t)
    assert np.array_equal(ds.Mean, ref.Mean) and ds.color_cam['f'] == ref.color_cam['f'] and ds.color_cam['c'] == ref.color_cam['c']
    assert ds.scene_floor_height == ref.scene_floor_height
    assert np.array_equal(ds.times_dst, np.arange(20) / 30.0) and ds.src_index.tolist() == list(range(20)) and not ds.gap.any()
    for ba, bb in zip(ds.batches(2), ref.batches(2)):
        assert set(ba) == set(bb) - {'gt_joints_scene_coord'} and (ba['frame_name'] == bb['frame_name']).all()
    item, ritem = ds[1], ref[1]
    assert set(item) == set(ritem) - {'gt_joints_scene_coord'}
    assert np.array_equal(item['motion_repr_noisy'], ritem['motion_repr_noisy']) and item['frame_name'] == ritem['frame_name']


# ---- (d) the tail ----------------------------------------------------------------------------------------------------------
def _synthetic_arrays(dataset, n, seed):
    keep = VT.N_FRAMES
    VT.N_FRAMES = n
    try:
        return VT.synthetic_tree_arrays(dataset, seed=seed)
    finally:
        VT.N_FRAMES = keep


@pytest.fixture(scope='module')
def logdir(tmp_path_factory):
    a = _synthetic_arrays('prox', 8, 0)
    return VT.write_tree(str(tmp_path_factory.mktemp('stats')), 'prox', a)['logdir']


def test_tail_clip_covers_the_end(logdir):
    from rohm_amd.data_loaders import clips, frames
    from rohm_amd.data_loaders.track import DataloaderTrack, read_track
    a = _synthetic_arrays('prox', 23, 1)
    track = track_from_tree(a, 'prox', -0.05)
    layer = _layer()
    kw = dict(body_model_path=layer, logdir=logdir, task='pose', clip_len=8, overlap_len=2, use_scene_floor_height=True, device=DEV)
    ds = DataloaderTrack(track, **kw)
    assert len(ds) == 4 and ds.clip_starts.tolist() == [0, 6, 12, 15] and len(ds.times_dst) == 23
    rec = read_track(track)
    joints_world, smplx_world = frames.frames_to_world(layer, rec['params'], rec['cam2world'], DEV)
    built = clips.build_clips(joints_world, smplx_world, 8, 2, up_axis='z', preset_floor_height=-0.05, stats=(ds.Mean, ds.Std), starts=[15])
    dv = ds._device_data
    for k, b in (('motion_repr_noisy', 'repr'), ('noisy_joints', 'cano_joints'), ('transf_matrix', 'transf_matrix'),
                 ('global_orient', 'global_orient'), ('transl', 'transl')):
        assert torch.equal(dv[k][3], built[b][0]), k
    assert torch.equal(dv['noisy_joints_scene_coord'][3], joints_world[15:23])
    kp = torch.from_numpy(rec['keypoints']).to(DEV)
    jv, vv = clips.visibility_masks(kp, torch.from_numpy(rec['mask_joint']).to(DEV), 8, 2, starts=[15])
    assert torch.equal(dv['mask_joint_vis'][3], jv[0]) and torch.equal(dv['mask_vec_vis'][3], vv[0])
    und = clips.undistort_keypoints(kp, a['cam_mtx'], a['cam_k'])
    assert torch.equal(dv['keypoints_2d'][3], und[15:23])
    assert ds.frame_name_list[3] == [str(s) for s in a['frame_names'][15:23]]
    for keep in ('first', 'last'):
        fc, ft, n = ds.export_plan(keep)
        assert n == 23 and (ds.clip_starts[fc] + ft).tolist() == list(range(23))          # every frame exactly once
    assert ds.export_plan()[0].tolist() == [0] * 8 + [1] * 6 + [2] * 6 + [3] * 3
    drop = DataloaderTrack(track, tail='drop', **kw)
    assert len(drop) == 3 and drop.clip_starts.tolist() == [0, 6, 12]
    for k in dv:
        assert torch.equal(drop._device_data[k], dv[k][:3]), k
    with pytest.raises(ValueError, match='least recording length'):
        DataloaderTrack(track_from_tree(a, 'prox', -0.05, n=7), **kw)


# ---- (e) gaps reach the masks ------------------------------------------------------------------------------------------------
def holed_25fps_track(a, n30, n25, hole, floor_height=-0.05):
    """A `video_tree` PROX recording of n30 frames at 30 fps, resampled on the host (the restatement) to n25 frames at 25 fps,
    with the frames `hole` lost; confidences 0.3 .. 1 and a mask of ones, so that only gaps hide joints."""
    t30 = np.arange(n30) / 30.0
    t25 = np.arange(n25) / 25.0
    assert t25[-1] <= t30[-1]
    src = track_from_tree(a, 'prox', floor_height)
    p = np.concatenate([src[k].astype(np.float64) for k in ('global_orient', 'transl', 'betas', 'body_pose')], axis=1)
    kp = src['keypoints_2d'].copy()
    kp[..., 2] = 0.3 + 0.7 * kp[..., 2]
    r = TR.resample(t30, np.ones(n30, bool), p, kp, None, t25, 1.0)
    valid = np.ones(n25, bool)
    valid[hole] = False
    out = dict(src, fps=25.0, keypoints_2d=r['keypoints'], mask_joint=np.ones((n25, 25), np.float32), valid=valid,
               frame_names=np.array(['cam_%04d' % i for i in range(n25)]))
    for k, (lo, hi) in (('global_orient', (0, 3)), ('transl', (3, 6)), ('betas', (6, 16)), ('body_pose', (16, 79))):
        out[k] = r['params'][:, lo:hi].astype(np.float32)
        out[k][hole] = np.nan
    return out


def test_gaps_reach_the_visibility_masks(logdir):
    import clips_ref as CR
    from rohm_amd.data_loaders.track import DataloaderTrack
    a = _synthetic_arrays('prox', 30, 2)
    hole = [9, 10, 11, 12, 13]
    track = holed_25fps_track(a, 30, 24, hole)
    ds = DataloaderTrack(track, body_model_path=_layer(), logdir=logdir, task='pose', clip_len=8, overlap_len=2, device=DEV)
    n = len(ds.times_dst)
    assert n == 28 and ds.clip_starts.tolist() == [0, 6, 12, 18, 20]
    # the gap is exactly the 30 fps frames strictly between source frames 8 and 14
    want_gap = (ds.times_dst > 8 / 25.0 + 1e-9) & (ds.times_dst < 14 / 25.0 - 1e-9)
    assert np.array_equal(ds.gap.astype(bool), want_gap) and want_gap.sum() == 7
    assert set(ds.src_index[want_gap].tolist()) == {8} and not np.isin(ds.src_index, hole).any()
    idx = ds.clip_starts[:, None] + np.arange(8)[None]
    jv, vv = ds._device_data['mask_joint_vis'].cpu().numpy(), ds._device_data['mask_vec_vis'].cpu().numpy()
    assert np.array_equal(jv == 0, np.broadcast_to(want_gap[idx][..., None], jv.shape))       # all 22 joints, at exactly the gap frames
    in_gap = want_gap[idx]
    assert in_gap[1].any() and not in_gap[1].all()                                              # a window cut through the gap
    ref_jv, ref_vv = CR.visibility_masks(np.zeros((22, 3)), np.ones(22))
    assert np.array_equal(vv[in_gap], np.broadcast_to(ref_vv.astype(np.float32), vv[in_gap].shape))
    assert (vv[~in_gap] == 1).all()
    assert not ds._device_data['keypoints_2d'].cpu().numpy()[in_gap][..., 2].any()
    assert all(torch.isfinite(v).all() for v in ds._device_data.values())
    assert ds.frame_name_list[1] == ['cam_%04d' % i for i in ds.src_index[6:14]]


# ---- (g) export and the way back -----------------------------------------------------------------------------------------------
def test_export_back_onto_the_source_times(logdir):
    from rohm_amd.data_loaders.track import DataloaderTrack
    from rohm_amd.export import export_params, resample_params
    a = _synthetic_arrays('prox', 46, 5)
    hole = [0, 12, 13, 14, 15, 16, 36]
    track = holed_25fps_track(a, 46, 37, hole)
    layer = _layer()
    L = 17
    ds = DataloaderTrack(track, body_model_path=layer, logdir=logdir, task='pose', clip_len=L, overlap_len=2, device=DEV)
    assert len(ds.times_dst) == 41 and ds.clip_starts.tolist() == [0, 15, 24]
    plan = ds.export_plan(rows=L - 1)
    assert plan[2] == 40
    res = export_params(ds._device_data['motion_repr_noisy'], ds._device_data['transf_matrix'], layer, stats=ds, frame='camera',
                        cam2world=track['cam2world'], plan=plan[:2])
    assert len(res) == 40
    p30 = res.params79.cpu().numpy()
    ang = max(np.linalg.norm(p30[:, c:c + 3], axis=-1).max() for c in TR.ROT_COLS)
    rel = max(TR.geodesic(p30[:-1, c:c + 3], p30[1:, c:c + 3]).max() for c in TR.ROT_COLS)
    print(f'exported rotations: max angle {ang:.3f} rad, max between neighbours {rel:.3f} rad')
    assert ang <= 3.0 and rel <= 2.0                                                     # where the restatement is held to scipy
    times_from = ds.times_dst[:40]
    span = slice(1, 36)                                                                  # first .. last source frame with a fit
    times_to = ds.times_src[span]
    back = resample_params(res, times_from, times_to, layer, gap_from=ds.gap[:40])
    assert len(back) == 35 and tuple(back.joints.shape) == (35, 22, 3) and torch.isfinite(back.params79).all()
    want = TR.resample(times_from, np.ones(40, bool), p30, None, None, times_to, 1.5 / 30.0)
    _compare({'params': back.params79, 'src_index': back.src_index, 'gap': want['gap']}, want, 'export_back')      # gap: next line
    assert np.array_equal(back.gap, want['gap'] | ds.gap[:40][want['src_index']]) and np.array_equal(back.times, times_to)
    assert back.gap[11:16].all() and not back.gap[:10].any()                             # the hole of the source is flagged
    # the recomputed joints are the body model's on the resampled parameters, and stay near the loader's input there
    from rohm_amd.data_loaders import frames
    j = frames.noisy_clip_joints(layer, {'global_orient': back.global_orient, 'transl': back.transl, 'betas': back.betas,
                                         'body_pose': back.body_pose}, DEV)
    assert torch.equal(j, back.joints)
    # a source time that is a 30 fps time comes back as that row's bits: source frame 1 is times_dst[0]
    assert torch.equal(back.params79[0], res.params79[0])


# ---- (f) the driver end to end ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def body_dir(tmp_path_factory):
    """SMPLX_NEUTRAL.npz in the released layout from the synthetic model (as tests/test_gpu_drivers.py)."""
    t = synth.synthetic_smplx_tensors(0)
    V = t['v_template'].shape[0]
    kt = np.stack([np.array(synth.SMPLX_PARENTS), np.arange(55)]).astype(np.int64)
    kt[0, 0] = 2 ** 32 - 1
    d = tmp_path_factory.mktemp('body')
    np.savez(str(d / 'SMPLX_NEUTRAL.npz'), v_template=t['v_template'].numpy(), shapedirs=t['shapedirs'].numpy(),
             posedirs=t['posedirs'].numpy().T.reshape(V, 3, 486), J_regressor=t['J_regressor'].numpy(), kintree_table=kt,
             weights=t['lbs_weights'].numpy(), f=np.zeros((4, 3), np.int64))
    return str(d)


@pytest.fixture(scope='module')
def scene(tmp_path_factory):
    """The 50-frame synthetic PROX recording of tests/test_gpu_drivers.py with random checkpoints next to its statistics."""
    a = _synthetic_arrays('prox', 50, 3)
    paths = VT.write_tree(str(tmp_path_factory.mktemp('prox50')), 'prox', a)
    ck = {}
    for k, sd in (('posenet', synth.posenet_state_dict(0)), ('trajnet', synth.trajnet_state_dict(1, trajcontrol=False)),
                  ('control', synth.trajnet_state_dict(2, trajcontrol=True))):
        ck[k] = os.path.join(paths['logdir'], f'model_{k}.pt')
        torch.save(sd, ck[k])
    return a, paths, ck


def _common(body_dir, ck, save_root, seed='4'):
    return ['--body_model_path', body_dir, '--model_path_posenet', ck['posenet'], '--model_path_trajnet', ck['trajnet'],
            '--model_path_trajnet_control', ck['control'], '--diffusion_steps_posenet', '6', '--diffusion_steps_trajnet', '4',
            '--sample_iter', '2', '--save_root', save_root, '--seed', seed, '--clip_len', '17', '--batch_size', '2']


def _load(path):
    with open(path, 'rb') as f:
        return pickle.load(f)


def test_track_driver_is_the_prox_driver_at_30_fps(scene, body_dir, tmp_path):
    from rohm_amd.drivers import results as R
    from rohm_amd.drivers.__main__ import main
    a, paths, ck = scene
    rec = str(a['recording_name'])
    floors = tmp_path / 'floors.json'
    floors.write_text('{"%s": -0.05}' % str(a['scene_name']))
    ref = main(['prox_egobody', '--dataset', 'prox', '--dataset_root', paths['base_dir'], '--init_root', paths['init_root'],
                '--recording_name', rec, '--floor_heights', str(floors)] + _common(body_dir, ck, str(tmp_path / 'ref')))
    track = str(tmp_path / 'walk.npz')
    np.savez(track, **track_from_tree(a, 'prox', -0.05))
    out = main(['track', '--track', track, '--tail', 'drop'] + _common(body_dir, ck, str(tmp_path / 'res')))
    assert out['path'].endswith('test_track_grad_True_iter_2_iter2trajnoisy_False_iter2posenoisy_False_earlystop_True_seed_4/' + rec + '.pkl')
    got, want = _load(out['path']), _load(ref['path'])
    assert list(got)[:len(want)] == list(want) and got['recording_name'] == rec
    assert list(got)[len(want):] == ['times_dst', 'src_index', 'gap', 'clip_starts', 'times_src', 'valid', 'source_frame_names', 'cam2world']
    assert got['motion_repr_rec_list'].shape == (3, 15, 294)
    for k in R.SCENE_PICKLE_KEYS:
        if isinstance(want.get(k), np.ndarray):
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k          # bit for bit, every array
    assert got['clip_starts'].tolist() == [0, 15, 30] and len(got['times_dst']) == 50 and not got['gap'].any()
    # refusals that say why
    with pytest.raises(ValueError, match='no ground truth'):
        main(['track', '--track', track, '--evaluate'] + _common(body_dir, ck, str(tmp_path / 'res')))
    bare = {k: v for k, v in track_from_tree(a, 'prox', -0.05).items() if k != 'keypoints_2d'}
    np.savez(str(tmp_path / 'bare.npz'), **bare)
    with pytest.raises(ValueError, match='keypoints_2d'):
        main(['track', '--track', str(tmp_path / 'bare.npz')] + _common(body_dir, ck, str(tmp_path / 'res')))


def test_track_driver_and_export_on_a_25_fps_track_with_a_hole(scene, body_dir, tmp_path):
    from rohm_amd.drivers.__main__ import main
    from rohm_amd.export import main as export_main
    a, paths, ck = scene
    hole = [0, 17, 18, 19, 20, 21]
    track = str(tmp_path / 'cam25.npz')
    td = holed_25fps_track(a, 50, 40, hole)
    np.savez(track, **td)
    out = main(['track', '--track', track] + _common(body_dir, ck, str(tmp_path / 'res'), seed='6'))
    got = _load(out['path'])
    n30 = len(got['times_dst'])
    assert n30 == 46 and got['clip_starts'].tolist() == [0, 15, 29]                  # 1/25 s .. 39/25 s; the tail clip ends at the end
    assert got['motion_repr_rec_list'].shape == (3, 15, 294)
    for k in ('motion_repr_rec_list', 'rec_ric_data_rec_list_from_smpl', 'rec_ric_data_rec_list_from_abs_traj', 'trans_scene2cano_list'):
        assert np.isfinite(got[k]).all(), k
    i0, _, _, gap = TR.brackets(np.arange(40) / 25.0, td['valid'], got['times_dst'], 0.06)
    assert np.array_equal(got['gap'], gap.astype(np.uint8)) and np.array_equal(got['src_index'], i0) and 6 <= gap.sum() <= 8
    assert got['valid'].sum() == 34 and np.array_equal(got['times_dst'], 1 / 25.0 + np.arange(46) / 30.0)
    # gaps arrived in the saved masks: the second clip holds frames 15 .. 29 of the pose stage
    assert gap[15:30].any() and np.array_equal((got['mask_joint_vis_list'][1] == 0).all(axis=-1), gap[15:30])
    # ... and the way back: one parameter row per source frame between the first and the last fit, holes included
    common = ['--dataset', 'track', '--saved_data_path', out['path'], '--body_model_path', body_dir, '--clip_len', '17']
    assert export_main(common + ['--out', str(tmp_path / 'src'), '--times', 'source', '--frame', 'camera']) == 0
    z = np.load(str(tmp_path / 'src' / str(a['recording_name']) / 'smplx_params.npz'))
    assert z['global_orient'].shape == (39, 3) and z['body_pose'].shape == (39, 63) and z['joints'].shape == (39, 22, 3)
    assert np.array_equal(z['times'], np.arange(1, 40) / 25.0) and z['frame_names'].tolist() == ['cam_%04d' % i for i in range(1, 40)]
    assert all(np.isfinite(z[k]).all() for k in ('global_orient', 'transl', 'betas', 'body_pose', 'joints'))
    assert z['gap'][16:21].all() and not z['gap'][:15].any() and str(z['coordinate_frame']) == 'camera'
    # ... or on the 30 fps grid: the tail clip's rows end two frames before the grid does (the pose stage keeps clip_len - 2)
    assert export_main(common + ['--out', str(tmp_path / 'g30'), '--times', '30fps']) == 0
    z30 = np.load(str(tmp_path / 'g30' / str(a['recording_name']) / 'smplx_params.npz'))
    assert z30['transl'].shape == (44, 3) and np.array_equal(z30['times'], got['times_dst'][:44]) and np.array_equal(z30['gap'], got['gap'][:44])
