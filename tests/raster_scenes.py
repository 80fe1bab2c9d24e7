"""TEST INFRASTRUCTURE ONLY: synthetic bodies with a face list, a walk in front of an OpenCV camera and a small scene, for
tests/test_gpu_raster.py and scripts/bench_occlusion.py."""
import numpy as np
import torch

import raster_ref as rr
from rohm_amd.utils import synth

N_FRAMES = 64


def sphere_body(seed=0, n_lat=48, n_lon=64):
    """Synthetic SMPL-X tensors whose vertices lie on an ellipsoid around the synthetic joint tree (synthetic bodies have
    no faces: the sphere's triangulation is skinned), each vertex owned by its nearest joint, smooth skinning weights."""
    sv, sf = rr.uv_sphere(n_lat, n_lon, 1.0, (0.0, 0.0, 0.0))
    V = len(sv)
    t = synth.synthetic_smplx_tensors(seed, num_verts=V)
    jpos = (t['J_regressor'].double() @ t['v_template'].double()).numpy()
    lo, hi = jpos.min(0), jpos.max(0)
    vt = sv.astype(np.float64) * ((hi - lo) * 0.5 * 1.15 + 0.05) + (hi + lo) * 0.5
    d2 = ((vt[:, None, :] - jpos[None]) ** 2).sum(-1)
    owner = d2.argmin(1)
    jr = (owner[None, :] == np.arange(len(jpos))[:, None]) + 0.002
    jr = jr / jr.sum(1, keepdims=True)
    w = np.exp(-(d2 - d2.min(1, keepdims=True)) / (2 * 0.12 ** 2))
    w /= w.sum(1, keepdims=True)
    t = dict(t)
    t['v_template'] = torch.from_numpy(vt.astype(np.float32))
    t['J_regressor'] = torch.from_numpy(jr.astype(np.float32))
    t['lbs_weights'] = torch.from_numpy(w.astype(np.float32))
    return t, sf


def _six_d_to_mat(x6):
    a, b = x6[..., 0::2].astype(np.float64), x6[..., 1::2].astype(np.float64)
    b1 = a / np.linalg.norm(a, axis=-1, keepdims=True)
    b2 = b - (b1 * b).sum(-1, keepdims=True) * b1
    b2 /= np.linalg.norm(b2, axis=-1, keepdims=True)
    return np.stack([b1, b2, np.cross(b1, b2)], -1)          # columns


def _mat_to_aa(R):
    ang = np.arccos(np.clip((np.trace(R, axis1=-2, axis2=-1) - 1) / 2, -1, 1))
    ax = np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1)
    n = np.linalg.norm(ax, axis=-1, keepdims=True)
    return ax / np.maximum(n, 1e-12) * ang[..., None]


def walking_params(tensors, n=N_FRAMES, seed=5):
    """SMPL-X parameters of `n` frames of synth.walking_motion, stood upright 3 m in front of an OpenCV camera and
    walking across (and partly out of) its field of view."""
    mean, std = synth.synthetic_stats(0)
    # the facing direction comes from the plain synthetic body (the sphere body's hip and shoulder joints need not differ)
    x = synth.walking_motion(seed, 1, n, mean, std, synth.synthetic_smplx_tensors(0, num_verts=2000)).numpy()[0] * std + mean
    up = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]], dtype=np.float64)                     # z up -> y down, z forward
    Rg = up @ _six_d_to_mat(x[:, 7:13])
    Rb = _six_d_to_mat(x[:, 154:280].reshape(n, 21, 6))
    j0 = (tensors['J_regressor'].double() @ tensors['v_template'].double()).numpy()[0]
    sweep = np.linspace(-3.1, 3.1, n)
    pelvis = np.stack([sweep + 0.3 * x[:, 16], 0.15 + 0.2 * x[:, 18], 3.0 + 0.6 * x[:, 17]], -1)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return {'transl': f32(pelvis - j0), 'global_orient': f32(_mat_to_aa(Rg)), 'body_pose': f32(_mat_to_aa(Rb).reshape(n, 63)),
            'betas': f32(np.tile(x[:1, 280:290], (n, 1)))}


def scene_mesh():
    """A wall in front of the right part of the walk and a table (top and front panel) in front of the lower body on the left; nothing
    on the far left.  Coordinates are multiples of 2^-10 m, so an exact rigid transform moves them exactly."""
    wall = rr.quad((0.3125, -2.0, 2.25), (4.0, -2.0, 2.1875), (4.0, 2.0, 2.1875), (0.3125, 2.0, 2.25))
    top = rr.quad((-1.75, 0.25, 1.5), (0.125, 0.25, 1.5), (0.125, 0.25, 2.25), (-1.75, 0.25, 2.25))
    front = rr.quad((-1.75, 0.25, 2.25), (0.125, 0.25, 2.25), (0.125, 2.0, 2.25), (-1.75, 2.0, 2.25))
    return rr.merge(wall, top, front)


def write_npz(path, tensors, faces):
    V = tensors['v_template'].shape[0]
    pd = tensors['posedirs'].numpy()                                                  # [486, V * 3]
    kin = np.stack([np.asarray(tensors['parents'].numpy(), dtype=np.int64), np.arange(len(tensors['parents']))])
    np.savez(path, v_template=tensors['v_template'].numpy(), shapedirs=tensors['shapedirs'].numpy(),
             posedirs=pd.T.reshape(V, 3, -1), J_regressor=tensors['J_regressor'].numpy(), kintree_table=kin,
             weights=tensors['lbs_weights'].numpy(), f=faces.astype(np.int64))
