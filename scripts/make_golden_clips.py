"""Golden vectors of the test-time clip builder and loader -> tests/golden/clips.npz, tests/golden/video_loader.npz.

clips.npz: the reference's own `cano_seq_smplx` / `cano_seq_smplx_egobody` (joints, parameters, transf_matrix) and the
294 de-normalised channels of its `get_repr_smplx` on every clip of `rohm_amd.utils.synth.synthetic_recording` (N = 48,
L = 16, overlap 2; z and y up; with and without a preset floor), plus one degenerate clip (N = L = 16, the hips and
shoulders of frames 5 and 9 moved onto the pelvis's xy: the reference yields NaN there).

video_loader.npz: the reference's own `DataloaderVideo` on a synthetic 20-frame PROX tree and EgoBody tree
(clip_len 8, overlap 2 -> 3 clips), task 'pose' and task 'traj' with repr_abs_only: the tree's contents as arrays and every
item of every clip.  The body model is the oracle's (registered with `refload.set_body_model`).  cv2 is a stub where this
runs: for PROX the stub gets an `undistortPoints` that calls the test restatement (tests/clips_ref.py), so that fixture
pins everything EXCEPT the undistortion arithmetic.

The reference is imported through oracle.refload; none of its text is here.  Needs a RoHM checkout at
oracle.refload.REF_ROOT; run once where it exists, commit only the .npz files:
    python scripts/make_golden_clips.py
"""
import json
import os
import pickle
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle import geometry as G  # noqa: E402
from oracle import refload  # noqa: E402
from rohm_amd.utils import synth  # noqa: E402
import clips_ref as CR  # noqa: E402
import video_tree as VT  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')


def ref_clip(ref, pos, world, up_axis, preset):
    mr = ref.motion_repr
    cano_fn = mr.cano_seq_smplx if up_axis == 'z' else mr.cano_seq_smplx_egobody
    prm = {k: v.copy() for k, v in CR.split_world(world).items()}
    cano, cp, tm = cano_fn(positions=pos.copy(), smplx_params_dict=prm, preset_floor_height=preset, return_transf_mat=True)
    d = mr.get_repr_smplx(positions=cano, smplx_params_dict=cp, feet_vel_thre=5e-5)
    full = np.concatenate([d[k] for k in ref.other_utils.REPR_LIST], axis=-1)
    return cano, cp, tm, full


def golden_clips(ref):
    out = {'seed': np.int64(CR.CLIP_SEED), 'N': np.int64(CR.CLIP_N), 'L': np.int64(CR.CLIP_L), 'overlap': np.int64(CR.CLIP_OVERLAP)}
    for up_axis in ('z', 'y'):
        jw, world = synth.synthetic_recording(CR.CLIP_SEED, CR.CLIP_N, up_axis)
        for with_preset in (False, True):
            preset = CR.clip_preset(jw, up_axis) if with_preset else None
            rows = [ref_clip(ref, jw[s:s + CR.CLIP_L], world[s:s + CR.CLIP_L], up_axis, preset)
                    for s in CR.window_starts(CR.CLIP_N, CR.CLIP_L, CR.CLIP_OVERLAP)]
            p = f"{up_axis}_{'preset' if with_preset else 'min'}_"
            out[p + 'cano_joints'] = np.stack([r[0] for r in rows])
            out[p + 'global_orient'] = np.stack([r[1]['global_orient'] for r in rows])
            out[p + 'transl'] = np.stack([r[1]['transl'] for r in rows])
            out[p + 'transf_matrix'] = np.stack([r[2] for r in rows])
            out[p + 'repr'] = np.stack([r[3] for r in rows])
            out[p + 'preset'] = np.float64(preset if with_preset else np.nan)
            fc = out[p + 'repr'][..., 290:]
            print(p, 'contact means', fc.mean(axis=(0, 1)).round(2), 'margin', CR.contact_margin(out[p + 'cano_joints']),
                  'min |across_xy|', RD_min_across(out[p + 'cano_joints']), 'nan', int(np.isnan(out[p + 'repr']).sum()))
    jw, world = synth.synthetic_recording(CR.CLIP_SEED, CR.CLIP_L, 'z', degenerate_frames=CR.DEGENERATE_FRAMES)
    cano, cp, tm, full = ref_clip(ref, jw, world, 'z', None)
    out['degenerate_repr'], out['degenerate_cano_joints'] = full[None], cano[None]
    nan = np.isnan(full)
    print('degenerate: NaN channels per frame', {int(t): np.flatnonzero(nan[t]).tolist()[:6] for t in np.flatnonzero(nan.any(1))})
    path = os.path.join(GOLD, 'clips.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


def RD_min_across(cano):
    from oracle import rederive as RD
    return float(np.min(RD.facing_margin(cano)[0]))


def _jsonable(v):
    return v.tolist() if isinstance(v, np.ndarray) else v


def golden_video_loader(ref):
    import importlib
    import torch
    body = G.BodyModel(synth.synthetic_smplx_tensors(0))
    refload.set_body_model(body)
    cv2 = sys.modules['cv2']
    cv2.undistortPoints = lambda src, cameraMatrix, distCoeffs, P: CR.undistort_pixels(src, cameraMatrix, distCoeffs)[:, None]
    dv = importlib.import_module('data_loaders.dataloader_video')
    out = {}
    for dataset in ('prox', 'egobody'):
        spec = VT.synthetic_tree_arrays(dataset)
        for k, v in spec.items():
            out[f'{dataset}_tree_{k}'] = v
        with tempfile.TemporaryDirectory() as tmp:
            paths = VT.write_tree(tmp, dataset, spec)
            table = getattr(ref.other_utils, f'{dataset}_floor_height')
            scene = str(spec['scene_name'])
            assert scene in table, (scene, sorted(table))
            out[f'{dataset}_floor_height'] = np.float64(table[scene])
            for task, abs_only in (('pose', False), ('traj', True)):
                for use_floor in (False, True):
                    ds = dv.DataloaderVideo(dataset=dataset, init_root=paths['init_root'], base_dir=paths['base_dir'],
                                            body_model_path='unused', recording_name=str(spec['recording_name']),
                                            use_scene_floor_height=use_floor, repr_abs_only=abs_only, task=task,
                                            overlap_len=VT.OVERLAP, clip_len=VT.CLIP_LEN, logdir=paths['logdir'], device='cpu')
                    p = f"{dataset}_{task}_{'floor' if use_floor else 'min'}_"
                    out[p + 'len'] = np.int64(len(ds))
                    for attr in ('body_feat_dim', 'traj_feat_dim', 'pose_feat_dim', 'n_samples', 'clip_len'):
                        out[p + attr] = np.int64(getattr(ds, attr))
                    out[p + 'scene_floor_height'] = np.float64(ds.scene_floor_height)
                    for i in range(len(ds)):
                        item = ds[i]
                        for k, v in item.items():
                            if k == 'cano_smplx_params_dict':
                                for kk, vv in v.items():
                                    out[f'{p}item{i}_params_{kk}'] = np.asarray(vv)
                            elif k == 'frame_name':
                                out[f'{p}item{i}_frame_name'] = np.array(v)
                            else:
                                out[f'{p}item{i}_{k}'] = np.asarray(v)
                    print(p, len(ds), sorted(item.keys()))
    path = os.path.join(GOLD, 'video_loader.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


def main():
    if not refload.available():
        raise SystemExit(f'needs the reference checkout at {refload.REF_ROOT}')
    ref = refload.load()
    what = sys.argv[1:] or ['clips', 'video_loader']
    if 'clips' in what:
        golden_clips(ref)
    if 'video_loader' in what:
        golden_video_loader(ref)


if __name__ == '__main__':
    main()
