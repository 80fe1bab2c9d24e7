"""Test-time clips of a PROX / EgoBody recording, built on the device (csrc/clips.hip).

`data_loaders/dataloader_video.py::create_body_repr` (:373-403) canonicalises every clip of a recording
(`cano_seq_smplx` / `cano_seq_smplx_egobody` + `update_globalRT_for_smplx`) and computes its 294-channel motion
representation (`get_repr_smplx`) one clip at a time in host numpy / scipy; `__getitem__` (:441-484) undistorts the
OpenPose keypoints and assembles the visibility masks per item.  The three functions here do that for all clips of a
recording in one launch each, reading the windows in place from what `frames.frames_to_world` returns."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .._lib import RohmHipError, check, lib, ptr, require_hip, stream_ptr

UP_AXES = {'z': 2, 'y': 1}


def n_clips(n_frames, clip_len, overlap_len):
    """Number of windows of the reference's `while 1:` loop (dataloader_video.py:167-179)."""
    step = clip_len - overlap_len
    if step <= 0:
        raise ValueError(f'overlap_len ({overlap_len}) must be smaller than clip_len ({clip_len})')
    return 0 if n_frames < clip_len else (n_frames - clip_len) // step + 1


def _starts_tensor(starts, n_frames, clip_len, device):
    """Explicit window starts -> int32 device tensor.  Host values are range-checked here; a device tensor is trusted
    (no synchronisation), the kernels answer NaN for a window that leaves the recording."""
    if torch.is_tensor(starts) and starts.is_cuda:
        if starts.dim() != 1 or starts.dtype not in (torch.int32, torch.int64):
            raise ValueError('starts must be a 1-D int32 / int64 tensor')
        return starts.to(dtype=torch.int32).contiguous()
    s = np.asarray(starts.cpu() if torch.is_tensor(starts) else starts)
    if s.ndim != 1 or (s.size and not np.issubdtype(s.dtype, np.integer)):
        raise ValueError('starts must be a 1-D sequence of integers')
    if s.size and (s.min() < 0 or s.max() + clip_len > n_frames):
        raise ValueError(f'starts {s.tolist()} with clip_len {clip_len} leave the {n_frames} frames of the recording')
    return torch.as_tensor(s.astype(np.int32), device=device)


def _check_clip_len(clip_len):
    if not isinstance(clip_len, (int, np.integer)) or not 2 <= clip_len <= 800:
        raise ValueError(f'clip_len must be an integer in [2, 800], got {clip_len!r}')


def _windows(starts, n_frames, clip_len, overlap_len, device):
    if starts is None:
        return None, n_clips(n_frames, clip_len, overlap_len)
    st = _starts_tensor(starts, n_frames, clip_len, device)
    return st, int(st.shape[0])


def _stats_tensors(stats, device):
    if stats is None:
        return None, None
    mean, std = (torch.as_tensor(np.asarray(s, dtype=np.float32) if not torch.is_tensor(s) else s).to(
        device=device, dtype=torch.float32).contiguous() for s in stats)
    if mean.shape != (294,) or std.shape != (294,):
        raise ValueError('stats must be (Mean [294], Std [294])')
    return mean, std


def build_clips(joints_world, smplx_world, clip_len, overlap_len=2, up_axis='z', preset_floor_height=None, stats=None,
                starts=None, params_f64=False):
    """All clips of a recording: canonicalise, re-express the SMPL-X parameters, compute the motion representation.

    joints_world [N,22,3] float32 and smplx_world [N,79] float64: the two device tensors `frames_to_world` returns.
    Clip c covers frames start_c .. start_c + clip_len - 1 with start_c = c * (clip_len - overlap_len), or `starts[c]`
    when `starts` is given.  up_axis 'z' (PROX, AMASS: `cano_seq_smplx`) or 'y' (EgoBody: `cano_seq_smplx_egobody`).
    preset_floor_height: the scene's floor instead of the clip's lowest joint (0.0 counts as None, as in the
    reference).  stats = (Mean, Std) [294] normalises the representation.

    Returns a dict of device tensors (float32): 'repr' [C, clip_len-1, 294], 'cano_joints' [C, clip_len, 22, 3],
    'global_orient' / 'transl' [C, clip_len, 3] (canonical; betas and body_pose pass through), 'transf_matrix'
    [C,4,4] (scene -> canonical), and 'starts' [C] int32.  params_f64=True adds 'orient_transl64' [C, clip_len, 6]: the
    canonical global_orient and transl in float64, as the AMASS loader keeps them; the other outputs do not change."""
    require_hip(joints_world, smplx_world)
    _check_clip_len(clip_len)
    if up_axis not in UP_AXES:
        raise ValueError(f"up_axis must be 'z' or 'y', got {up_axis!r}")
    if joints_world.dim() != 3 or joints_world.shape[1:] != (22, 3) or joints_world.dtype != torch.float32:
        raise ValueError(f'joints_world must be float32 [N,22,3], got {joints_world.dtype} {tuple(joints_world.shape)}')
    N = joints_world.shape[0]
    if smplx_world.shape != (N, 79) or smplx_world.dtype != torch.float64:
        raise ValueError(f'smplx_world must be float64 [{N},79], got {smplx_world.dtype} {tuple(smplx_world.shape)}')
    device = joints_world.device
    if smplx_world.device != device:
        raise ValueError('joints_world and smplx_world must be on the same device')
    st, n = _windows(starts, N, clip_len, overlap_len, device)
    mean, std = _stats_tensors(stats, device)
    L = int(clip_len)
    f32 = dict(device=device, dtype=torch.float32)
    out = {'repr': torch.empty(n, L - 1, 294, **f32), 'cano_joints': torch.empty(n, L, 22, 3, **f32),
           'global_orient': torch.empty(n, L, 3, **f32), 'transl': torch.empty(n, L, 3, **f32),
           'transf_matrix': torch.empty(n, 4, 4, **f32),
           'starts': st if st is not None else torch.arange(n, device=device, dtype=torch.int32) * (L - int(overlap_len))}
    if params_f64:
        out['orient_transl64'] = torch.empty(n, L, 6, device=device, dtype=torch.float64)
    if n == 0:
        return out
    nbytes = lib().rohm_clips_scratch_bytes(n, L)
    scratch = torch.empty(nbytes, device=device, dtype=torch.uint8) if nbytes else None
    has_preset = preset_floor_height is not None
    head = (ptr(joints_world.contiguous()), ptr(smplx_world.contiguous()), N, ptr(st), n, L, int(overlap_len), UP_AXES[up_axis],
            int(has_preset), float(preset_floor_height) if has_preset else 0.0, ptr(mean), ptr(std), ptr(out['repr']),
            ptr(out['cano_joints']), ptr(out['global_orient']), ptr(out['transl']), ptr(out['transf_matrix']))
    with torch.cuda.device(device):
        if params_f64:
            check(lib().rohm_clips_build_f64(*head, ptr(out['orient_transl64']), ptr(scratch), nbytes, stream_ptr(device)),
                  'rohm_clips_build_f64')
        else:
            check(lib().rohm_clips_build(*head, ptr(scratch), nbytes, stream_ptr(device)), 'rohm_clips_build')
    return out


def clips_repr(positions, params, stats=None, joint_noise=None, return_joints=False):
    """`get_repr_smplx` (feet_vel_thre 5e-5) of clips that are canonical already: positions [C,L,22,3] (device float32 or
    float64), params [C,L,79] float64 (global_orient, transl, betas, body_pose) -> [C, L-1, 294] float32.  The arithmetic
    the reference does in the joints' dtype follows the dtype of `positions`.  joint_noise [C,L,22,3] float64: the joints
    become float32(positions + joint_noise) first (the sep_noise items of the AMASS loader); return_joints=True also
    returns the float32 joints the representation was made of."""
    require_hip(positions, params, joint_noise)
    if positions.dim() != 4 or positions.shape[2:] != (22, 3) or positions.dtype not in (torch.float32, torch.float64):
        raise ValueError(f'positions must be float32 / float64 [C,L,22,3], got {positions.dtype} {tuple(positions.shape)}')
    n, L = int(positions.shape[0]), int(positions.shape[1])
    _check_clip_len(L)
    device = positions.device
    if params.shape != (n, L, 79) or params.dtype != torch.float64 or params.device != device:
        raise ValueError(f'params must be float64 [{n},{L},79] on {device}, got {params.dtype} {tuple(params.shape)}')
    if joint_noise is not None and (joint_noise.shape != positions.shape or joint_noise.dtype != torch.float64 or
                                    joint_noise.device != device):
        raise ValueError(f'joint_noise must be float64 {tuple(positions.shape)} on {device}')
    mean, std = _stats_tensors(stats, device)
    out = torch.empty(n, L - 1, 294, device=device, dtype=torch.float32)
    joints = torch.empty(n, L, 22, 3, device=device, dtype=torch.float32) if return_joints else None
    if n:
        nbytes = lib().rohm_clips_scratch_bytes(n, L)
        scratch = torch.empty(nbytes, device=device, dtype=torch.uint8) if nbytes else None
        with torch.cuda.device(device):
            check(lib().rohm_clips_repr(ptr(positions.contiguous()), int(positions.dtype == torch.float64), ptr(params.contiguous()),
                                        ptr(joint_noise.contiguous() if joint_noise is not None else None), n, L, ptr(mean),
                                        ptr(std), ptr(out), ptr(joints), ptr(scratch), nbytes, stream_ptr(device)),
                  'rohm_clips_repr')
    return (out, joints) if return_joints else out


def undistort_keypoints(keypoints, camera_mtx, dist_coeffs, image_width=1920):
    """dataloader_video.py:441-458 for keypoints [...,3] = (x, y, confidence) (device float32): mirror x, undistort
    as `cv2.undistortPoints(src, camera_mtx, dist, P=camera_mtx)` does (five iterations, k1 k2 p1 p2 k3), mirror back.
    camera_mtx [3,3] and dist_coeffs [5] are host values (`Color.json`'s 'camera_mtx' and 'k').  float32 result."""
    require_hip(keypoints)
    if keypoints.dim() < 1 or keypoints.shape[-1] != 3 or keypoints.dtype != torch.float32:
        raise ValueError(f'keypoints must be float32 [...,3], got {keypoints.dtype} {tuple(keypoints.shape)}')
    K = np.ascontiguousarray(np.asarray(camera_mtx, dtype=np.float64))
    k = np.ascontiguousarray(np.asarray(dist_coeffs, dtype=np.float64).reshape(-1))
    if K.shape != (3, 3) or k.shape != (5,):
        raise ValueError(f'camera_mtx must be [3,3] and dist_coeffs [5], got {K.shape} {k.shape}')
    kp = keypoints.contiguous()
    out = torch.empty_like(kp)
    with torch.cuda.device(kp.device):
        check(lib().rohm_keypoints_undistort(ptr(kp), kp.numel() // 3, K.ctypes.data_as(C.POINTER(C.c_double)),
                                             k.ctypes.data_as(C.POINTER(C.c_double)), float(image_width), ptr(out),
                                             stream_ptr(kp.device)), 'rohm_keypoints_undistort')
    return out


def visibility_masks(keypoints, mask_joint, clip_len, overlap_len=2, starts=None):
    """dataloader_video.py:462-484 for all clips: keypoints [N,22,3] (confidence last) and mask_joint [N, >=22] (the
    depth-occlusion mask, 1 = visible; both device float32) -> (mask_joint_vis [C, clip_len, 22], mask_vec_vis
    [C, clip_len, 294]) float32, windows as in `build_clips`."""
    require_hip(keypoints, mask_joint)
    if not isinstance(clip_len, (int, np.integer)) or clip_len < 1:
        raise ValueError(f'clip_len must be a positive integer, got {clip_len!r}')
    if keypoints.dim() != 3 or keypoints.shape[1:] != (22, 3) or keypoints.dtype != torch.float32:
        raise ValueError(f'keypoints must be float32 [N,22,3], got {keypoints.dtype} {tuple(keypoints.shape)}')
    N = keypoints.shape[0]
    if mask_joint.dim() != 2 or mask_joint.shape[0] != N or mask_joint.shape[1] < 22 or mask_joint.dtype != torch.float32:
        raise ValueError(f'mask_joint must be float32 [{N}, >=22], got {mask_joint.dtype} {tuple(mask_joint.shape)}')
    device = keypoints.device
    if mask_joint.device != device:
        raise ValueError('keypoints and mask_joint must be on the same device')
    st, n = _windows(starts, N, clip_len, overlap_len, device)
    L = int(clip_len)
    jv = torch.empty(n, L, 22, device=device, dtype=torch.float32)
    vv = torch.empty(n, L, 294, device=device, dtype=torch.float32)
    if n:
        with torch.cuda.device(device):
            check(lib().rohm_visibility_masks(ptr(keypoints.contiguous()), ptr(mask_joint.contiguous()), mask_joint.shape[1],
                                              N, ptr(st), n, L, int(overlap_len), ptr(jv), ptr(vv), stream_ptr(device)),
                  'rohm_visibility_masks')
    return jv, vv
