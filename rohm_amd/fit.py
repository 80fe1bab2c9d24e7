"""Fit SMPL-X to 3-D joints: from a skeleton recording to a track.

A track (`rohm_amd.data_loaders.track`) holds per-frame SMPL-X parameters.  A depth-camera body tracker, multi-view
triangulation, a 3-D pose lifter or marker mocap reduced to joint centres give a skeleton instead.  This module fits the
body model's pose (and, on request, one shape for the recording) to such joints on the device and writes a track:

    python -m rohm_amd.fit --skeleton skeleton.npz --body_model_path body_models/smplx_model --out raw.npz --json report.json
    python -m rohm_amd.floor --track raw.npz --body_model_path body_models/smplx_model --out calibrated.npz
    python -m rohm_amd.drivers track --track calibrated.npz ...

The rule (kernels in csrc/fit.hip, stated in full in include/rohm_hip.h, restated in tests/fit_ref.py).  Per frame the unknowns
are the axis-angles theta of joints 0..21 and a translation t; `rohm_fit_pose` minimises

    E = sum_j c_j |p_j(theta, beta) + t - y_j|^2 + sum_k w_prior[k] |theta_k|^2 + w_smooth sum_{k=1..21} |theta_k - m_k|^2

by Levenberg-Marquardt with an analytic Jacobian, one workgroup per frame.  p_j are `rohm_smplx_joints`' joints, y_j the given
joints, c_j their confidences (0 for a joint that is missing or not finite), m_k the mean of the neighbouring frames' last
solution.  A frame starts from the rotation that takes the rest body's hips-and-neck triad onto the observed one; a frame that
cannot (a hip or the neck is missing) starts from the nearest fitted frame; a frame with fewer than `min_joints` joints is left
out (`valid` false).  With `fit_shape`, `rohm_fit_shape_moments` gives the sums of the linear least-squares problem for one beta
at the fixed poses, the host solves the 10 x 10 system, and poses and shape alternate.

Limits: the joints must be SMPL's (BODY_25 is mapped through `OPENPOSE_TO_SMPL`, as a track's keypoints are); joints of another
convention sit elsewhere in the body and should be given confidence 0.  One person.  No hands, face or expression.  The twist
about a bone and the wrists' rotations are not observable from 22 joints: the prior holds them at zero.  `w_prior`, `w_smooth`
and `ridge` are chosen on the synthetic body with the float64 restatement, not fitted to real recordings."""
from __future__ import annotations

import argparse
import functools
import json
import sys

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr

NJ, NX, NROT, N_MOMENTS = 22, 69, 66, 66
SKELETON_KEYS = ('joints_3d', 'joint_conf', 'betas', 'fps', 'times')
PASS_THROUGH = ('cam2world', 'keypoints_2d', 'mask_joint', 'up_axis', 'focal_length', 'camera_center', 'camera_mtx', 'dist_coeffs',
                'image_width', 'floor_height', 'frame_names', 'recording_name')
W_SMOOTH, RIDGE = 1e-2, 1e-5
# SMPL joints that OPENPOSE_TO_SMPL fills with a neighbour's BODY_25 joint (spine1, spine2 from MidHip, spine3 from Neck, the collars
# from the shoulders): close enough for 2-D guidance, 10 - 20 cm off in 3-D.  A BODY_25 skeleton leaves them unobserved.
BODY25_PROXY = (3, 6, 9, 13, 14)


def default_w_prior():
    """0 for the root, 1e-4 for joints 1..19, 1e-2 for the wrists (20, 21): they have no observed child among the 22 joints, so
    their rotation is not observable.  Chosen on the synthetic body with the float64 restatement, not on real recordings."""
    w = np.full(NJ, 1e-4)
    w[0] = 0.0
    w[20:] = 1e-2
    return w


class FitResult:
    """params [N,69] float64 (the axis-angles of joints 0..21, then transl; zeros where not valid), betas [10] float64, valid [N]
    bool, report [N,6] float64 (status 0 skipped / 1 fitted / 2 no start, E at the start and at the end of the last pass,
    accepted iterations, final lambda, the weighted rms residual in metres), warm_started [N] bool, energy_history (a list, with
    fit_shape: sum of E over the valid frames + ridge n |beta|^2 before the first shape step and after every round; else None)."""
    __slots__ = ('params', 'betas', 'valid', 'report', 'warm_started', 'energy_history')

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])

    def summary(self):
        v = self.valid
        rms = self.report[v, 5]
        return {'frames': int(len(v)), 'fitted': int(v.sum()), 'skipped': int((~v).sum()), 'warm_started': int(self.warm_started.sum()),
                'median_residual_m': float(np.median(rms)), 'worst_residual_m': float(rms.max()), 'worst_frame': int(np.flatnonzero(v)[rms.argmax()]),
                'betas': self.betas.tolist(), 'energy_history': self.energy_history}


# ---- the kernels' wrappers -----------------------------------------------------------------------------------------------------
_hip = functools.partial(_lib.hip_tensor, kernels='the fit kernels take')


def _observations(targets, conf):
    t = _hip(targets, 'targets').detach().float().contiguous()
    if t.dim() != 3 or tuple(t.shape[1:]) != (NJ, 3):
        raise ValueError(f'targets must be [N, 22, 3], got {list(t.shape)}')
    N = int(t.shape[0])
    c = None
    if conf is not None:
        c = _hip(conf, 'conf').detach().float().contiguous()
        if tuple(c.shape) != (N, NJ):
            raise ValueError(f'conf must be [{N}, 22], got {list(c.shape)}')
    return t, c, N


def _rows(x, name, N):
    return _lib.hip_rows(x, name, (N, NX), kernels='the fit kernels take')


def fit_pose(nat, targets, conf, betas, init=None, prev=None, w_prior=None, w_smooth=0.0, iters=20, min_joints=6, want_normal=False):
    """`rohm_fit_pose`: nat a native body handle (`body_model.native_for`), targets [N,22,3] float32, conf [N,22] float32 or
    None, betas [N,10] float32, init / prev [N,69] float64 or None, w_prior [22] float64 (HIP tensors) -> (params [N,69], report
    [N,6], normal [N,69,70] or None) float64 on the device."""
    t, c, N = _observations(targets, conf)
    b = _hip(betas, 'betas').detach().float().contiguous()
    if tuple(b.shape) != (N, 10):
        raise ValueError(f'betas must be [{N}, 10], got {list(b.shape)}')
    i0, p0 = _rows(init, 'init', N), _rows(prev, 'prev', N)
    wp = torch.from_numpy(default_w_prior()).to(t.device) if w_prior is None else _hip(w_prior, 'w_prior').detach().double().contiguous()
    if tuple(wp.shape) != (NJ,):
        raise ValueError(f'w_prior must be [22], got {list(wp.shape)}')
    params = torch.empty(N, NX, device=t.device, dtype=torch.float64)
    report = torch.empty(N, 6, device=t.device, dtype=torch.float64)
    normal = torch.empty(N, NX, NX + 1, device=t.device, dtype=torch.float64) if want_normal else None
    with torch.cuda.device(t.device):
        check(lib().rohm_fit_pose(nat.handle, ptr(t), ptr(c), ptr(b), ptr(i0), ptr(p0), ptr(wp), float(w_smooth), int(iters), int(min_joints),
                                  N, ptr(params), ptr(report), ptr(normal), stream_ptr(t.device)), 'rohm_fit_pose')
    return params, report, normal


def shape_moments(nat, targets, conf, params, use):
    """`rohm_fit_shape_moments`: targets, conf as `fit_pose`, params [N,69] float64, use [N] bool or uint8 (HIP tensors) ->
    (per_frame [N,66], out [66]) float64 on the device."""
    t, c, N = _observations(targets, conf)
    p = _rows(params, 'params', N)
    u = _hip(use, 'use').detach().to(torch.uint8).contiguous()
    if tuple(u.shape) != (N,):
        raise ValueError(f'use must be [{N}], got {list(u.shape)}')
    rows = torch.empty(N, N_MOMENTS, device=t.device, dtype=torch.float64)
    out = torch.zeros(N_MOMENTS, device=t.device, dtype=torch.float64)
    with torch.cuda.device(t.device):
        check(lib().rohm_fit_shape_moments(nat.handle, ptr(t), ptr(c), ptr(p), ptr(u), N, ptr(rows), ptr(out), stream_ptr(t.device)),
              'rohm_fit_shape_moments')
    return rows, out


# ---- host logic (float64 numpy) ---------------------------------------------------------------------------------------------------
def solve_shape(moments, ridge, n_frames):
    """beta [10] of (M + ridge n I) beta = v from `shape_moments`' totals [66]."""
    m = np.asarray(moments, dtype=np.float64).reshape(N_MOMENTS)
    M = np.zeros((10, 10))
    M[np.triu_indices(10)] = m[:55]
    M = M + np.triu(M, 1).T
    return np.linalg.solve(M + float(ridge) * n_frames * np.eye(10), m[55:65])


def shape_energy(moments, beta, ridge, n_frames):
    """sum c |y - a - A beta|^2 + ridge n |beta|^2 from the totals: the data energy as a quadratic in beta."""
    m = np.asarray(moments, dtype=np.float64).reshape(N_MOMENTS)
    M = np.zeros((10, 10))
    M[np.triu_indices(10)] = m[:55]
    M = M + np.triu(M, 1).T
    b = np.asarray(beta, dtype=np.float64)
    return float(b @ M @ b - 2.0 * m[55:65] @ b + m[65] + ridge * n_frames * (b @ b))


def nearest_fitted(times, fitted, need):
    """For every frame in `need` the index of the fitted frame nearest in time (the earlier one on ties)."""
    idx = np.flatnonzero(fitted)
    return {int(i): int(idx[np.argmin(np.abs(times[idx] - times[i]))]) for i in np.flatnonzero(need)}


def _native(body_model, device):
    from .body_model import native_for
    from .data_loaders.dataloader_video import _body_model
    return native_for(_body_model(body_model, 'neutral', device), device)


def fit_joints(joints, conf=None, betas=None, times=None, fit_shape=False, shape_rounds=3, ridge=RIDGE, w_prior=None, w_smooth=W_SMOOTH,
               iters=20, smooth_passes=1, min_joints=6, body_model='body_models/smplx_model', device='cuda:0', log=None):
    """SMPL-X pose (and one shape) from joints [N,22,3] in SMPL order, metres, any frame of reference -> `FitResult`.

    conf [N,22] (default ones; a joint that is missing, not finite or of another convention gets 0), betas [10] (default zeros:
    the mean shape; the start of the shape fit), times [N] seconds (default the frame index; used only to find the nearest
    fitted frame).  1. every frame is fitted on its own from the torso triad; 2. frames that have no start (status 2) are run
    once more from the parameters of the nearest fitted frame; frames still not fitted are `valid = False`, and a recording
    without a fitted frame raises ValueError; 3. with `fit_shape`, `shape_rounds` times: the shape that minimises the data term
    at the fixed poses plus `ridge` n |beta|^2, then the poses again from their last solution -- both steps lower sum E + ridge n
    |beta|^2, which `energy_history` records; 4. `smooth_passes` times: every frame again from its last solution with
    `w_smooth` pulling its body pose to its neighbours' last solution.  `w_prior` (default `default_w_prior()`), `w_smooth` and
    `ridge` are chosen on the synthetic body with the float64 restatement, not on real recordings.  There is no CPU path."""
    log = log or (lambda s: None)
    device = torch.device(device)
    y = np.asarray(joints, dtype=np.float32)
    if y.ndim != 3 or y.shape[1:] != (NJ, 3) or y.shape[0] < 1:
        raise ValueError(f'joints must be [N, 22, 3] with N >= 1, got {y.shape}')
    N = y.shape[0]
    if conf is not None and np.asarray(conf).shape != (N, NJ):
        raise ValueError(f'conf must be [{N}, 22], got {np.asarray(conf).shape}')
    ts = np.arange(N, dtype=np.float64) if times is None else np.asarray(times, dtype=np.float64).reshape(-1)
    if ts.shape != (N,):
        raise ValueError(f'times must be [{N}], got {ts.shape}')
    beta = np.zeros(10) if betas is None else np.asarray(betas, dtype=np.float64).reshape(-1)
    if beta.shape != (10,):
        raise ValueError(f'betas must be [10], got {beta.shape}')
    wp = default_w_prior() if w_prior is None else np.asarray(w_prior, dtype=np.float64).reshape(-1)
    if wp.shape != (NJ,):
        raise ValueError(f'w_prior must be [22], got {wp.shape}')
    nat = _native(body_model, device)
    yd = torch.from_numpy(y).to(device)
    cd = None if conf is None else torch.from_numpy(np.asarray(conf, dtype=np.float32)).to(device)
    wd = torch.from_numpy(wp).to(device)

    def beta_rows(n):
        return torch.from_numpy(np.repeat(beta.astype(np.float32)[None], n, axis=0)).to(device)

    def run(init=None, prev=None, w=0.0, rows=None):
        sel = (lambda t: t) if rows is None else (lambda t: None if t is None else t[rows].contiguous())
        p, r, _ = fit_pose(nat, sel(yd), sel(cd), beta_rows(N if rows is None else len(rows)), init=sel(init), prev=sel(prev), w_prior=wd,
                           w_smooth=w, iters=iters, min_joints=min_joints)
        return p.cpu().numpy(), r.cpu().numpy()

    def solution(params, valid):
        return torch.from_numpy(np.where(valid[:, None], params, np.nan)).to(device)

    params, report = run()
    status = report[:, 0].astype(np.int64)
    log(f'pass 1: {int((status == 1).sum())} of {N} frames fitted, {int((status == 2).sum())} without a start, {int((status == 0).sum())} skipped')
    warm = np.zeros(N, bool)
    need = status == 2
    if need.any() and (status == 1).any():
        src = nearest_fitted(ts, status == 1, need)
        rows = np.array(sorted(src), dtype=np.int64)
        init = np.full((N, NX), np.nan)
        init[rows] = params[[src[int(i)] for i in rows]]
        p2, r2 = run(init=torch.from_numpy(init).to(device), rows=torch.from_numpy(rows).to(device))
        params[rows], report[rows] = p2, r2
        warm[rows] = r2[:, 0] == 1
        log(f'warm start: {int(warm.sum())} of {len(rows)} frames fitted from their nearest fitted frame')
    valid = report[:, 0] == 1
    if not valid.any():
        raise ValueError(f'no frame could be fitted: {int((status == 0).sum())} of {N} frames have fewer than min_joints={min_joints} joints and '
                         f'{int((status == 2).sum())} have no hips-and-neck triad to start from')
    n = int(valid.sum())
    history = None
    if fit_shape:
        history = [float(report[valid, 2].sum() + ridge * n * (beta @ beta))]
        use = torch.from_numpy(valid.astype(np.uint8)).to(device)
        for rnd in range(int(shape_rounds)):
            _, tot = shape_moments(nat, yd, cd, torch.from_numpy(params).to(device), use)
            tot = tot.cpu().numpy()
            cand = solve_shape(tot, ridge, n).astype(np.float32).astype(np.float64)      # the kernels read float32 betas
            if shape_energy(tot, cand, ridge, n) <= shape_energy(tot, beta, ridge, n):
                beta = cand
            params, report = run(init=solution(params, valid))
            history.append(float(report[valid, 2].sum() + ridge * n * (beta @ beta)))
            log(f'shape round {rnd + 1}: sum E + ridge n |beta|^2 = {history[-1]:.6e}')
    for k in range(int(smooth_passes)):
        sol = solution(params, valid)
        params, report = run(init=sol, prev=sol, w=w_smooth)
        log(f'smoothing pass {k + 1}: median residual {np.median(report[valid, 5]) * 1000.0:.2f} mm')
    params = np.where(valid[:, None], params, 0.0)
    return FitResult(params=params, betas=beta, valid=valid, report=report, warm_started=warm, energy_history=history)


# ---- skeleton file -> track ---------------------------------------------------------------------------------------------------------
def read_skeleton(skeleton):
    """Validate a skeleton (an .npz path or a dict) -> (joints [N,22,3] float32, conf [N,22] float32 or None, betas [10] or None,
    times [N] float64, the pass-through entries).  Required: joints_3d [N,22,3] (SMPL order) or [N,25,3] (BODY_25, mapped through
    `OPENPOSE_TO_SMPL`; the SMPL joints `BODY25_PROXY`, which that map fills with a neighbouring BODY_25 joint, get confidence 0) and
    exactly one of fps and times.  Optional: joint_conf [N,22|25], betas [10] and the track's own
    optional entries (`PASS_THROUGH`), which are handed on untouched.  Any other key is refused by name."""
    from .data_loaders.dataloader_video import OPENPOSE_TO_SMPL
    d = _lib.npz_dict(skeleton)
    unknown = sorted(set(d) - set(SKELETON_KEYS) - set(PASS_THROUGH))
    if unknown:
        raise ValueError(f'skeleton: unknown keys {unknown}; a skeleton has {list(SKELETON_KEYS)} and may carry {list(PASS_THROUGH)}')
    if 'joints_3d' not in d:
        raise ValueError("skeleton: missing ['joints_3d']")
    j = np.asarray(d['joints_3d'], dtype=np.float32)
    if j.ndim != 3 or j.shape[0] < 1 or j.shape[1:] not in ((NJ, 3), (25, 3)):
        raise ValueError(f'skeleton: joints_3d must be [N,22,3] (SMPL order) or [N,25,3] (BODY_25) with N >= 1, got {j.shape}')
    N, K = j.shape[0], j.shape[1]
    conf = None
    if 'joint_conf' in d:
        conf = np.asarray(d['joint_conf'], dtype=np.float32)
        if conf.shape != (N, K):
            raise ValueError(f'skeleton: joint_conf must be [{N},{K}] like joints_3d, got {conf.shape}')
    if K == 25:
        j = j[:, OPENPOSE_TO_SMPL[0:NJ]]
        conf = np.ones((N, NJ), np.float32) if conf is None else conf[:, OPENPOSE_TO_SMPL[0:NJ]].copy()
        conf[:, list(BODY25_PROXY)] = 0.0
    if ('fps' in d) == ('times' in d):
        raise ValueError('skeleton: give exactly one of fps and times')
    if 'fps' in d:
        fps = np.asarray(d['fps'], dtype=np.float64)
        if fps.size != 1 or not np.isfinite(fps).all() or float(fps.reshape(-1)[0]) <= 0:
            raise ValueError(f'skeleton: fps must be one positive number, got {d["fps"]!r}')
        times = np.arange(N, dtype=np.float64) / float(fps.reshape(-1)[0])
    else:
        times = np.asarray(d['times'], dtype=np.float64)
        if times.shape != (N,) or not np.isfinite(times).all() or (np.diff(times) <= 0).any():
            raise ValueError(f'skeleton: times must be [{N}], finite and strictly increasing')
    betas = None
    if 'betas' in d:
        betas = np.asarray(d['betas'], dtype=np.float64).reshape(-1)
        if betas.shape != (10,) or not np.isfinite(betas).all():
            raise ValueError(f'skeleton: betas must be 10 finite numbers, got shape {np.asarray(d["betas"]).shape}')
    return np.ascontiguousarray(j), conf, betas, times, {k: d[k] for k in PASS_THROUGH if k in d}


def fit_track(skeleton, body_model='body_models/smplx_model', device='cuda:0', return_result=False, **kw):
    """A skeleton (`read_skeleton`) -> a track dict with only `TRACK_KEYS`: the fitted global_orient [N,3], transl [N,3],
    body_pose [N,63], betas [10] (float32) and valid [N], fps or times as given, and the skeleton's pass-through entries.  With
    cam2world among them `read_track` accepts it; without, `floor.calibrate_track` does.  `kw` goes to `fit_joints`."""
    d = _lib.npz_dict(skeleton)
    joints, conf, betas, times, extra = read_skeleton(d)
    res = fit_joints(joints, conf=conf, betas=betas, times=times, body_model=body_model, device=device, **kw)
    p = res.params.astype(np.float32)
    track = dict(global_orient=p[:, :3], body_pose=p[:, 3:NROT], transl=p[:, NROT:], betas=res.betas.astype(np.float32), valid=res.valid.copy())
    track['fps' if 'fps' in d else 'times'] = d['fps'] if 'fps' in d else d['times']
    track.update(extra)
    return (track, res) if return_result else track


# ---- the tool ------------------------------------------------------------------------------------------------------------------------
OPTIONS = (('iters', int, 20, 'Levenberg-Marquardt iterations per pass'),
           ('smooth_passes', int, 1, 'passes that pull every frame to its neighbours\' last solution'),
           ('w_smooth', float, W_SMOOTH, 'weight of the smoothing term (per rad^2, against the data term in m^2)'),
           ('prior_scale', float, 1.0, 'multiplies the default pose prior (default_w_prior); 0 leaves what the joints do not determine to the damping'),
           ('min_joints', int, 6, 'a frame with fewer observed joints is left out (valid = false)'),
           ('shape_rounds', int, 3, 'with --fit_shape: alternations of shape and pose'),
           ('ridge', float, RIDGE, 'with --fit_shape: ridge on beta, per frame'))


def build_parser():
    ap = argparse.ArgumentParser(prog='python -m rohm_amd.fit', description='fit SMPL-X to a 3-D skeleton recording and write a track')
    ap.add_argument('--skeleton', type=str, required=True, help='the skeleton file (.npz): joints_3d, fps or times, optionally joint_conf, betas')
    ap.add_argument('--out', type=str, required=True, help='write the track here (.npz)')
    ap.add_argument('--body_model_path', type=str, default='body_models/smplx_model')
    ap.add_argument('--fit_shape', action='store_true', help='fit one shape (betas) for the recording as well')
    for name, typ, default, text in OPTIONS:
        ap.add_argument('--' + name, type=typ, default=default, help=text)
    ap.add_argument('--json', type=str, default='', help='write the report here')
    ap.add_argument('--device', type=str, default='cuda:0')
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    kw = {name: getattr(args, name) for name, _, _, _ in OPTIONS}
    opts = dict(kw, fit_shape=args.fit_shape)
    kw['w_prior'] = default_w_prior() * kw.pop('prior_scale')
    try:
        track, res = fit_track(args.skeleton, body_model=args.body_model_path, device=args.device, return_result=True, fit_shape=args.fit_shape,
                               log=lambda s: print('[rohm_amd.fit] ' + s), **kw)
    except ValueError as e:
        raise SystemExit(f'{args.skeleton}: {e}')
    s = res.summary()
    print(' --------------- SMPL-X fitted to the skeleton -------------')
    print('frames fitted / skipped:     %d / %d of %d (%d from a warm start)' % (s['fitted'], s['skipped'], s['frames'], s['warm_started']))
    print('residual, median / worst:    %.2f / %.2f mm (frame %d)' % (s['median_residual_m'] * 1e3, s['worst_residual_m'] * 1e3, s['worst_frame']))
    if s['energy_history'] is not None:
        print('energy per shape round:      ' + ' -> '.join('%.5e' % e for e in s['energy_history']))
    np.savez(args.out, **track)
    print(f'[rohm_amd.fit] wrote {args.out}' + ('' if 'cam2world' in track else ' (no cam2world: python -m rohm_amd.floor finds one)'))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump({'skeleton': args.skeleton, 'summary': s, 'options': opts,
                       'report': [[None if not np.isfinite(v) else float(v) for v in row] for row in res.report]}, f, indent=1)
            f.write('\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
