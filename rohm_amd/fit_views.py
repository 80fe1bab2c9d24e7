"""Fit SMPL-X to 2-D keypoints by reprojection: from one calibrated camera, or several, to a track.

`rohm_amd.multiview` turns several views into a skeleton that `rohm_amd.fit` takes; one camera with a 2-D detector (a phone, a
webcam with OpenPose) had no way in, and the chain drops what a single view sees and every view's own uncertainty.  This module
fits the body straight to the pixels of every view, on the device:

    python -m rohm_amd.fit_views --views views.npz --body_model_path body_models/smplx_model --out raw.npz --json report.json
    python -m rohm_amd.floor --track raw.npz --body_model_path body_models/smplx_model --out calibrated.npz
    python -m rohm_amd.drivers track --track calibrated.npz ...

The rule (kernel in csrc/fit_views.hip, stated in full in include/rohm_fit_views.h, restated in tests/fit_views_ref.py).  Per frame
the unknowns are the axis-angles theta of joints 0..21 and a translation t; `rohm_fit_views_pose` minimises

    E = sum_v sum_j c_vj rho(|r_vj|^2) + sum_k w_prior[k] |theta_k|^2 + w_smooth sum_{k=1..21} |theta_k - m_k|^2 + w_smooth_t |t - m_t|^2

by Levenberg-Marquardt with an analytic Jacobian, one workgroup per frame.  r_vj is the reprojection error in pixels of joint j in
view v against its undistorted detection, c_vj the detection's confidence, rho the Geman-McClure function with scale `sigma_px`
(plain least squares at 0): the mis-detection of one view saturates and does not drag the body.  m are the means of the
neighbouring frames' last solution.  A joint that a single view sees still pulls on the body, and a narrow baseline weighs as
little as it should.

The start.  With two or more views: `multiview.triangulate`, then `fit.fit_pose` on the triangulated joints.  With one view (and
for frames where that chain yields nothing): two candidates, a body that stands upright in the reference view facing the camera
and one that turns its back, each with its translation solved in closed form by the kernel; both run, as 2 N problems in one
launch, and the smaller final energy wins.

Limits.  One person; synchronised (`python -m rohm_amd.sync`), calibrated views; 1 to 16 of them.  The shape is GIVEN (`betas`,
default the mean shape), not fitted: with one view scale and depth are not separable -- a larger body further away gives the same pixels -- so a wrong shape
turns into a wrong distance.  There is no learned pose prior.  With several views this is a refinement with millimetre accuracy
on the synthetic body (measured with the restatement at 2 px of noise: 7 mm in the mean and 20 mm in the worst joint with two
views, 4 mm and 13 mm with four); with ONE view the pixels are met (0.5 px) but the depth along the viewing ray is held by the
body's size and the pose prior alone: on noise-free synthetic input of a body that faces the camera to within 0.5 rad, 27 mm in
the mean and 45 mm in the worst joint (profiles/fit_views_parity.json); six walking frames as a BODY_25 file come out 65 mm off
in the mean and 40 cm in the worst joint at 0.9 px, a limb whose depth one view cannot see.  A monocular result is a rough track with correct pixels, the kind of input the
denoiser exists for, not a measurement.

`w_prior`, `w_smooth`, `w_smooth_t` and `sigma_px` are chosen, not fitted to recordings: `fit`'s defaults, which weigh against
metres squared, are carried to pixels squared by (f / z)^2 at f = 1000 px and z = 3.5 m (8e4, rounded to 1e5); one view gets a
tenth of the pose prior of several: a prior straightens the limbs, which a single view can only answer by moving the whole body
along the viewing ray (with the restatement on the noise-free synthetic body: 18 cm of mean joint error at ten times the prior of
several views, 10 cm at the same, 2.7 cm at a tenth)."""
from __future__ import annotations

import argparse
import functools
import json
import sys

import numpy as np
import torch

from . import _lib, fit, multiview
from ._lib import check, lib, ptr, stream_ptr

NJ, NX, NROT, NREPORT, MAX_VIEWS = 22, 69, 66, 8, 16
CONF_MIN, MIN_OBS, SIGMA_PX, W_SMOOTH, W_SMOOTH_T = multiview.CONF_MIN, 12, 30.0, 1e3, 1e3
PRIOR_PX = 1e5                       # fit.default_w_prior() (per m^2) in px^2: (f / z)^2 at f = 1000 px, z = 3.5 m, rounded
PRIOR_ONE_VIEW = 0.1                 # one view: a tenth of the pose prior of several (see above)


def default_w_prior(n_views):
    """`fit.default_w_prior()` carried to pixels (times 1e5), a tenth of that for a single view.  Chosen, not fitted."""
    return fit.default_w_prior() * PRIOR_PX * (PRIOR_ONE_VIEW if n_views == 1 else 1.0)


class FitViewsResult:
    """params [N,69] float64 (the axis-angles of joints 0..21, then transl, in the world frame of the cameras; zeros where not
    valid), betas [10] float64, valid [N] bool, report [N,8] float64 (status 0 too few observations / 1 fitted / 2 no finite start /
    3 no usable start, E at the start and at the end of the last pass, accepted iterations, final lambda, the weighted rms
    reprojection error in px, the number of observations, the smallest depth), resid [V,N,22] float64 (the reprojection error in
    px per view and joint, NaN where unobserved), warm_started [N] bool (the start came from triangulation and `fit.fit_pose`),
    back_turned [N] bool (the monocular candidate that turns its back won)."""
    __slots__ = ('params', 'betas', 'valid', 'report', 'resid', 'warm_started', 'back_turned')

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])

    def summary(self):
        v = self.valid
        rms = self.report[v, 5]
        return {'frames': int(len(v)), 'fitted': int(v.sum()), 'skipped': int((~v).sum()), 'warm_started': int(self.warm_started.sum()),
                'back_turned': int(self.back_turned.sum()), 'median_reprojection_px': float(np.median(rms)), 'worst_reprojection_px': float(rms.max()),
                'worst_frame': int(np.flatnonzero(v)[rms.argmax()]), 'betas': self.betas.tolist()}


# ---- the kernel's wrapper ------------------------------------------------------------------------------------------------------
_hip = functools.partial(_lib.hip_tensor, kernels='the fit_views kernel takes')


def _rows(x, name, N):
    return _lib.hip_rows(x, name, (N, NX), kernels='the fit_views kernel takes')


def fit_views_pose(nat, keypoints, cams, betas, init, prev=None, w_prior=None, w_smooth=0.0, w_smooth_t=0.0, sigma_px=0.0, conf_min=CONF_MIN,
                   iters=20, min_obs=MIN_OBS, want_resid=True, want_normal=False):
    """`rohm_fit_views_pose`: nat a native body handle (`body_model.native_for`), keypoints [V,N,22,3] float32 (x, y in pixels as
    detected, confidence; SMPL joint order), cams [V,24] float64 (`multiview.pack_cameras`), betas [N,10] float32, init [N,69]
    float64 (a row whose translation is three NaN has it solved by the kernel), prev [N,69] float64 or None, w_prior [22] float64
    (HIP tensors) -> (params [N,69], report [N,8], resid [V,N,22] or None, normal [N,69,70] or None) float64 on the device.  One
    launch, no synchronisation, nothing read back; there is no CPU path."""
    kp = _hip(keypoints, 'keypoints').detach().float().contiguous()
    if kp.dim() != 4 or tuple(kp.shape[2:]) != (NJ, 3):
        raise ValueError(f'keypoints must be [V, N, 22, 3], got {list(kp.shape)}')
    V, N = int(kp.shape[0]), int(kp.shape[1])
    cm = _hip(cams, 'cams').detach().double().contiguous()
    if tuple(cm.shape) != (V, multiview.CAM):
        raise ValueError(f'cams must be [{V}, {multiview.CAM}] (pack_cameras), got {list(cm.shape)}')
    b = _hip(betas, 'betas').detach().float().contiguous()
    if tuple(b.shape) != (N, 10):
        raise ValueError(f'betas must be [{N}, 10], got {list(b.shape)}')
    if init is None:
        raise ValueError('init must be [N, 69]: rohm_fit_views_pose needs a start (start_rows gives the monocular ones)')
    i0, p0 = _rows(init, 'init', N), _rows(prev, 'prev', N)
    wp = torch.from_numpy(default_w_prior(V)).to(kp.device) if w_prior is None else _hip(w_prior, 'w_prior').detach().double().contiguous()
    if tuple(wp.shape) != (NJ,):
        raise ValueError(f'w_prior must be [22], got {list(wp.shape)}')
    dev = kp.device
    params = torch.empty(N, NX, device=dev, dtype=torch.float64)
    report = torch.empty(N, NREPORT, device=dev, dtype=torch.float64)
    resid = torch.empty(V, N, NJ, device=dev, dtype=torch.float64) if want_resid else None
    normal = torch.empty(N, NX, NX + 1, device=dev, dtype=torch.float64) if want_normal else None
    with torch.cuda.device(dev):
        check(lib().rohm_fit_views_pose(nat.handle, ptr(kp), ptr(cm), ptr(b), ptr(i0), ptr(p0), ptr(wp), float(w_smooth), float(w_smooth_t),
                                        float(sigma_px), float(conf_min), int(iters), int(min_obs), V, N, ptr(params), ptr(report), ptr(resid),
                                        ptr(normal), stream_ptr(dev)), 'rohm_fit_views_pose')
    return params, report, resid, normal


# ---- host logic (float64 numpy) ---------------------------------------------------------------------------------------------------
def _log_map(R):
    """Rotation matrix -> axis-angle, by the rule of csrc/fit_math.h's log_map64 (a half turn takes its axis from R + R^T)."""
    c = (R[0, 0] + R[1, 1] + R[2, 2] - 1.0) * 0.5
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = 0.5 * np.sqrt((v * v).sum())
    ang = np.arctan2(s, c)
    if s >= 1e-6 and c > -0.99:
        return v * (ang / (2.0 * s))
    if c > 0.0:
        return 0.5 * v
    i = int(np.argmax(np.diag(R)))
    n = np.zeros(3)
    n[i] = np.sqrt(max((R[i, i] - c) / (1.0 - c), 0.0))
    for j in range(3):
        if j != i:
            n[j] = 0.5 * (R[i, j] + R[j, i]) / ((1.0 - c) * n[i])
    sign = -1.0 if float(v @ n) < 0.0 else 1.0
    return sign * n / np.sqrt((n * n).sum()) * ang


def start_rows(cams, ref_view=0):
    """The two monocular starts -> [2,69] float64: root rotation R_ref^T diag(1, -1, -1) (upright in the reference view's image and
    facing its camera: the body model's y is up and its z is forward, a camera's y is down and its z looks away) and
    R_ref^T diag(-1, -1, 1) (back turned); the body pose is zero and the translation NaN, which the kernel solves."""
    cams = np.asarray(cams, dtype=np.float64)
    if cams.ndim != 2 or cams.shape[1] != multiview.CAM or not 0 <= int(ref_view) < cams.shape[0]:
        raise ValueError(f'start_rows: cams must be [V, {multiview.CAM}] and ref_view in [0, V), got {cams.shape} and {ref_view}')
    R = cams[int(ref_view), :9].reshape(3, 3)
    rows = np.zeros((2, NX))
    rows[:, NROT:] = np.nan
    rows[0, :3] = _log_map(R.T @ np.diag([1.0, -1.0, -1.0]))
    rows[1, :3] = _log_map(R.T @ np.diag([-1.0, -1.0, 1.0]))
    return rows


def fit_views(keypoints, cams, betas=None, init=None, ref_view=0, w_prior=None, w_smooth=W_SMOOTH, w_smooth_t=W_SMOOTH_T, sigma_px=SIGMA_PX,
              conf_min=CONF_MIN, iters=30, smooth_passes=1, min_obs=MIN_OBS, body_model='body_models/smplx_model', device='cuda:0', log=None):
    """SMPL-X pose from keypoints [V,N,22,3] (SMPL order; x, y in pixels as detected, confidence) of V calibrated views, cams
    [V,24] (`multiview.pack_cameras`) -> `FitViewsResult`, the parameters in the cameras' world frame.

    betas [10] is given (default zeros: the mean shape), not fitted: with one view scale and depth are not separable.  init
    [N,69] (optional) starts every frame where its row is finite.  Otherwise, 1. with V >= 2 the start is `multiview.triangulate`
    followed by `fit.fit_pose`; 2. with V == 1, and for the frames where step 1 yields nothing, the two `start_rows` run as 2 N
    problems in one launch and `torch.where` keeps the candidate with the smaller final energy (one that has no usable start
    loses); with V == 1 nothing is read back before the end.  3. `smooth_passes` times: every frame again from its last solution,
    `w_smooth` and `w_smooth_t` pulling its body pose and translation to its neighbours' last solution.  Frames that end without
    a fit are `valid = False`; a recording without one raises ValueError.  `w_prior` defaults to `default_w_prior(V)`; it,
    `w_smooth`, `w_smooth_t` and `sigma_px` are chosen on the synthetic body, not on real recordings.  There is no CPU path."""
    log = log or (lambda s: None)
    device = torch.device(device)
    kp = np.asarray(keypoints, dtype=np.float32)
    if kp.ndim != 4 or kp.shape[2:] != (NJ, 3) or kp.shape[1] < 1 or not 1 <= kp.shape[0] <= MAX_VIEWS:
        raise ValueError(f'keypoints must be [V, N, 22, 3] with 1 <= V <= {MAX_VIEWS} and N >= 1, got {kp.shape}')
    V, N = kp.shape[:2]
    cm = np.asarray(cams, dtype=np.float64)
    if cm.shape != (V, multiview.CAM):
        raise ValueError(f'cams must be [{V}, {multiview.CAM}] (pack_cameras), got {cm.shape}')
    beta = np.zeros(10) if betas is None else np.asarray(betas, dtype=np.float64).reshape(-1)
    if beta.shape != (10,):
        raise ValueError(f'betas must be [10], got {beta.shape}')
    wp = default_w_prior(V) if w_prior is None else np.asarray(w_prior, dtype=np.float64).reshape(-1)
    if wp.shape != (NJ,):
        raise ValueError(f'w_prior must be [22], got {wp.shape}')
    if init is not None and np.asarray(init).shape != (N, NX):
        raise ValueError(f'init must be [{N}, 69], got {np.asarray(init).shape}')
    starts = start_rows(cm, ref_view)
    nat = fit._native(body_model, device)
    kpd, camd, wd = torch.from_numpy(kp).to(device), torch.from_numpy(cm).to(device), torch.from_numpy(wp).to(device)
    bd = torch.from_numpy(np.repeat(beta.astype(np.float32)[None], 2 * N, axis=0)).to(device)
    opts = dict(w_prior=wd, sigma_px=sigma_px, conf_min=conf_min, iters=iters, min_obs=min_obs)
    nan = torch.full((N, NX), float('nan'), device=device, dtype=torch.float64)

    start = nan.clone() if init is None else torch.from_numpy(np.asarray(init, dtype=np.float64)).to(device)
    warm = torch.zeros(N, device=device, dtype=torch.bool)
    if V >= 2 and init is None:
        tri = multiview.triangulate(kpd, camd, conf_min=conf_min)
        p3, r3, _ = fit.fit_pose(nat, tri.joints.float(), tri.conf, bd[:N], iters=iters)
        warm = r3[:, 0] == 1
        start = torch.where(warm[:, None], p3, nan)
    usable = torch.isfinite(start).all(dim=1)
    back = torch.zeros(N, device=device, dtype=torch.bool)
    # (V == 1 without init: no host read; otherwise one flag is read, as fit_joints reads its statuses)
    mono = (V == 1 and init is None) or not bool(usable.all())
    if mono:
        both = torch.from_numpy(np.repeat(starts, N, axis=0)).to(device)                  # [2N,69]: N rows facing, N rows back turned
        p2, r2, s2, _ = fit_views_pose(nat, torch.cat([kpd, kpd], dim=1), camd, bd, both, **opts)
        inf = torch.full((), float('inf'), device=device, dtype=torch.float64)
        ea, eb = (torch.where(r2[q * N:(q + 1) * N, 0] == 1, r2[q * N:(q + 1) * N, 2], inf) for q in (0, 1))
        back = (eb < ea) & ~usable
        pm = torch.where(back[:, None], p2[N:], p2[:N])
        rm = torch.where(back[:, None], r2[N:], r2[:N])
        sm = torch.where(back[None, :, None], s2[:, N:], s2[:, :N])
    if V == 1 and init is None:
        params, report, resid = pm, rm, sm
    else:
        params, report, resid, _ = fit_views_pose(nat, kpd, camd, bd[:N], torch.where(usable[:, None], start, nan), **opts)
        if mono:
            params, report = torch.where(usable[:, None], params, pm), torch.where(usable[:, None], report, rm)
            resid = torch.where(usable[None, :, None], resid, sm)
    for _ in range(int(smooth_passes)):
        sol = torch.where((report[:, 0] == 1)[:, None], params, nan)
        params, report, resid, _ = fit_views_pose(nat, kpd, camd, bd[:N], sol, prev=sol, w_smooth=w_smooth, w_smooth_t=w_smooth_t, **opts)
    report_h = report.cpu().numpy()
    valid = report_h[:, 0] == 1
    log(f'{int(valid.sum())} of {N} frames fitted from {V} view{"s" if V > 1 else ""}; {int((report_h[:, 0] == 0).sum())} have fewer than '
        f'{min_obs} observations, {int((report_h[:, 0] >= 2).sum())} no usable start')
    if not valid.any():
        raise ValueError(f'no frame could be fitted: {int((report_h[:, 0] == 0).sum())} of {N} frames have fewer than min_obs={min_obs} '
                         f'observations and {int((report_h[:, 0] >= 2).sum())} have no usable start')
    return FitViewsResult(params=np.where(valid[:, None], params.cpu().numpy(), 0.0), betas=beta, valid=valid, report=report_h,
                          resid=resid.cpu().numpy(), warm_started=warm.cpu().numpy() & valid, back_turned=back.cpu().numpy() & valid)


# ---- views file -> track ---------------------------------------------------------------------------------------------------------------
def _undistorted(kp, K, dist):
    """One view's keypoints [N,K,3] with x, y undistorted (rule 1 of rohm_multiview.h) where they are finite."""
    out = np.array(kp, dtype=np.float32)
    if dist is None or not np.any(dist):
        return out
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    k1, k2, p1, p2, k3 = (float(x) for x in dist)
    with np.errstate(all='ignore'):
        x0, y0 = (out[..., 0].astype(np.float64) - cx) / fx, (out[..., 1].astype(np.float64) - cy) / fy
        x, y = x0, y0
        for _ in range(5):
            r2 = x * x + y * y
            icd = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
            dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
            dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
            x, y = (x0 - dx) * icd, (y0 - dy) * icd
        ok = np.isfinite(out[..., 0]) & np.isfinite(out[..., 1])
        out[..., 0] = np.where(ok, (fx * x + cx).astype(np.float32), out[..., 0])
        out[..., 1] = np.where(ok, (fy * y + cy).astype(np.float32), out[..., 1])
    return out


def fit_views_track(views, ref_view=0, betas=None, body_model='body_models/smplx_model', device='cuda:0', return_result=False, **kw):
    """A views file (`multiview.read_views`, here with one view or more) -> a track dict with only `TRACK_KEYS`.  BODY_25 keypoints
    are mapped through `OPENPOSE_TO_SMPL`, the joints `fit.BODY25_PROXY` at confidence 0.  The cameras are re-expressed relative to
    view `ref_view` on the host, so global_orient and transl come out in that camera's frame, as a track's are.  The track has
    global_orient [N,3], body_pose [N,63], transl [N,3], betas [10] (float32), valid [N], fps or times as given, keypoints_2d (the
    reference view's, undistorted), focal_length and camera_center (its intrinsics), frame_names and recording_name where given,
    and -- only when world_up_axis was given -- cam2world (the inverse of that view's world2cam), up_axis and floor_height.  `kw`
    goes to `fit_views`."""
    from .data_loaders.dataloader_video import OPENPOSE_TO_SMPL
    v = multiview.read_views(views, min_views=1)
    kp, W, K = v['keypoints'], v['world2cam'], v['camera_mtx']
    V, N = kp.shape[:2]
    if not 0 <= int(ref_view) < V:
        raise ValueError(f'ref_view must be in [0, {V}), got {ref_view}')
    ref = int(ref_view)
    kps = kp
    if kp.shape[2] == 25:
        kps = kp[:, :, OPENPOSE_TO_SMPL[0:NJ]].copy()
        kps[:, :, list(fit.BODY25_PROXY), 2] = 0.0
    cams = multiview.pack_cameras(K, W @ np.linalg.inv(W[ref])[None], v['dist_coeffs'])       # the world is now the reference camera
    res = fit_views(kps, cams, betas=betas, ref_view=ref, body_model=body_model, device=device, **kw)
    p = res.params.astype(np.float32)
    track = dict(global_orient=p[:, :3], body_pose=p[:, 3:NROT], transl=p[:, NROT:], betas=res.betas.astype(np.float32), valid=res.valid.copy())
    track[v['time_key']] = v[v['time_key']]
    track['keypoints_2d'] = _undistorted(kp[ref], K[ref], None if v['dist_coeffs'] is None else v['dist_coeffs'][ref])
    track['focal_length'] = np.array([K[ref, 0, 0], K[ref, 1, 1]])
    track['camera_center'] = np.array([K[ref, 0, 2], K[ref, 1, 2]])
    track.update({k: v[k] for k in ('frame_names', 'recording_name') if k in v})
    if v['world_up_axis'] is not None:
        track['cam2world'] = np.linalg.inv(W[ref])
        track['up_axis'] = v['world_up_axis']
        if v['floor_height'] is not None:
            track['floor_height'] = v['floor_height']
    return (track, res) if return_result else track


# ---- the tool ------------------------------------------------------------------------------------------------------------------------
OPTIONS = (('iters', int, 30, 'Levenberg-Marquardt iterations per pass'),
           ('smooth_passes', int, 1, 'passes that pull every frame to its neighbours\' last solution'),
           ('sigma_px', float, SIGMA_PX, 'scale of the robust function in pixels; 0 is plain least squares'),
           ('w_smooth', float, W_SMOOTH, 'weight of the pose smoothing (per rad^2, against the data term in px^2)'),
           ('w_smooth_t', float, W_SMOOTH_T, 'weight of the translation smoothing (per m^2, against the data term in px^2)'),
           ('prior_scale', float, 1.0, 'multiplies the default pose prior (default_w_prior)'),
           ('conf_min', float, CONF_MIN, 'a detection is observed when its confidence exceeds this'),
           ('min_obs', int, MIN_OBS, 'a frame with fewer observations over all views is left out (valid = false)'))


def build_parser():
    ap = argparse.ArgumentParser(prog='python -m rohm_amd.fit_views',
                                 description='fit SMPL-X to the 2-D keypoints of one or several calibrated cameras and write a track')
    ap.add_argument('--views', type=str, required=True, help='the views file (.npz): keypoints_2d, camera_mtx, world2cam or cam2world, fps or times')
    ap.add_argument('--out', type=str, required=True, help='write the track here (.npz)')
    ap.add_argument('--body_model_path', type=str, default='body_models/smplx_model')
    ap.add_argument('--ref_view', type=int, default=0, help='the track is in this view\'s camera frame and carries its keypoints')
    ap.add_argument('--betas', type=str, default='', help='a .npy or .npz (key betas) with the 10 shape coefficients; default the mean shape')
    for name, typ, default, text in OPTIONS:
        ap.add_argument('--' + name, type=typ, default=default, help=text + ' (chosen, not fitted)')
    ap.add_argument('--json', type=str, default='', help='write the report here')
    ap.add_argument('--device', type=str, default='cuda:0')
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    kw = {name: getattr(args, name) for name, _, _, _ in OPTIONS}
    opts = dict(kw, ref_view=args.ref_view)
    scale = kw.pop('prior_scale')
    betas = None
    if args.betas:
        loaded = np.load(args.betas, allow_pickle=False)
        betas = np.asarray(loaded['betas'] if hasattr(loaded, 'files') else loaded, dtype=np.float64).reshape(-1)
    try:
        n_views = multiview.read_views(args.views, min_views=1)['keypoints'].shape[0]
        track, res = fit_views_track(args.views, ref_view=args.ref_view, betas=betas, body_model=args.body_model_path, device=args.device,
                                     return_result=True, w_prior=default_w_prior(n_views) * scale,
                                     log=lambda s: print('[rohm_amd.fit_views] ' + s), **kw)
    except (ValueError, _lib.RohmHipError) as e:
        raise SystemExit(f'{args.views}: {e}')
    s = res.summary()
    print(' --------------- SMPL-X fitted to the keypoints of %d view%s -------------' % (n_views, '' if n_views == 1 else 's'))
    print('frames fitted / skipped:        %d / %d of %d (%d from triangulation, %d back turned)' % (s['fitted'], s['skipped'], s['frames'],
                                                                                                    s['warm_started'], s['back_turned']))
    print('reprojection, median / worst:   %.2f / %.2f px (frame %d)' % (s['median_reprojection_px'], s['worst_reprojection_px'], s['worst_frame']))
    if n_views == 1:
        print('one view: depth along the viewing ray is not observable without a learned prior; this is a rough track with correct pixels')
    np.savez(args.out, **track)
    print(f'[rohm_amd.fit_views] wrote {args.out}' + ('' if 'cam2world' in track else ' (no world_up_axis: python -m rohm_amd.floor finds the floor)'))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump({'views': args.views, 'summary': s, 'options': opts,
                       'report': [[None if not np.isfinite(x) else float(x) for x in row] for row in res.report]}, f, indent=1)
            f.write('\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
