"""Triangulate multi-view 2-D keypoints: from several calibrated, synchronised cameras to a skeleton.

`rohm_amd.fit` takes a 3-D skeleton.  A rig of cameras with a 2-D detector on each (any multi-camera lab; EgoBody's master and
four sub Kinects with their OpenPose files) gives 2-D keypoints per view instead.  Two or more views need no pose prior: the
step to a skeleton is geometry, done here in one launch for a whole recording:

    python -m rohm_amd.multiview --views views.npz --out skeleton.npz --json report.json
    python -m rohm_amd.fit --skeleton skeleton.npz --body_model_path body_models/smplx_model --out raw.npz
    python -m rohm_amd.floor --track raw.npz --body_model_path body_models/smplx_model --out calibrated.npz

The rule (kernels in csrc/multiview.hip, stated in full in include/rohm_multiview.h, restated in tests/multiview_ref.py).  Per
(frame, joint): the views whose detection is finite with a confidence above `conf_min` are undistorted (cv2.undistortPoints'
five iterations, no mirroring) and turned into rays; every pair of them whose rays meet at more than `min_angle_deg` proposes
the midpoint of their common perpendicular; the proposal whose own two views and most other views reproject within `tau_px`
wins (then the smaller confidence-weighted cost, then the lower pair index); its inliers are refined by `refine` Gauss-Newton
steps on the weighted reprojection error.  A mis-detection of one view (a left / right swap, another person, furniture) is
thrown out, not averaged in.  A point with fewer than two observed views, no proposal or fewer than `min_views` inliers has no
result: NaN joints with confidence 0, which `rohm_amd.fit` treats as missing.

`tau_px`, `conf_min`, `min_angle_deg` and `min_views` are stated parameters: chosen, not fitted to recordings.

Limits: synchronised cameras (per-view time offsets are not estimated here: `python -m rohm_amd.sync` first); one person
(detections are not associated across people); a calibrated rig (`python -m rohm_amd.rig` calibrates one from the keypoints
themselves); 2 to 16 views.  With
exactly three observed views and one mis-detection the counts tie at 2 and only the cost decides, which kept a few outliers
per hundred such points in the prototype of this rule: use `--min_views 3` where four or more cameras see the person."""
from __future__ import annotations

import argparse
import ctypes as C
import functools
import json
import sys

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr

CAM = 24
VIEW_KEYS = ('keypoints_2d', 'camera_mtx', 'world2cam', 'cam2world', 'dist_coeffs', 'fps', 'times', 'world_up_axis', 'floor_height',
             'frame_names', 'recording_name')
CONF_MIN, TAU_PX, MIN_ANGLE_DEG, MIN_VIEWS, REFINE = 0.2, 10.0, 2.0, 2, 3


def limits():
    """`rohm_mv_limits` -> (max_views, max_pairs)."""
    v, p = C.c_int(0), C.c_int(0)
    check(lib().rohm_mv_limits(C.byref(v), C.byref(p)), 'rohm_mv_limits')
    return v.value, p.value


class Triangulation:
    """joints [N,J,3] float64 (NaN where there is no result), conf [N,J] float32 (the mean confidence of the inliers, 0 where
    there is no result), report [N,J,4] float64 (the number of inliers, their weighted rms reprojection error in px, sigma_m:
    the standard deviation in metres for one pixel of noise, the number of observed views), inliers [N,J] int32 (bit v set when
    view v is an inlier), keypoints_und [V,N,J,3] float32 or None: tensors on the device of the keypoints."""
    __slots__ = ('joints', 'conf', 'report', 'inliers', 'keypoints_und')

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])


# ---- the kernels' wrappers -----------------------------------------------------------------------------------------------------
_TAKE = 'the multiview kernels take'
_hip = functools.partial(_lib.hip_tensor, kernels=_TAKE)


def keypoints_operand(keypoints, kernels):
    """keypoints [V,N,J,3] as a contiguous float32 HIP tensor -> (kp, V, N, J); `kernels` as `_lib.hip_tensor` takes it.  `rig` and
    `sync` check their operands here too."""
    kp = _lib.hip_tensor(keypoints, 'keypoints', kernels).detach().float().contiguous()
    if kp.dim() != 4 or kp.shape[3] != 3 or kp.shape[2] < 1:
        raise ValueError(f'keypoints must be [V, N, J, 3], got {list(kp.shape)}')
    V, N, J = (int(s) for s in kp.shape[:3])
    return kp, V, N, J


def views_operands(keypoints, cams, kernels):
    """`keypoints_operand` and cams [V,24] (`pack_cameras`) as a contiguous float64 HIP tensor -> (kp, cm, V, N, J)."""
    kp, V, N, J = keypoints_operand(keypoints, kernels)
    cm = _lib.hip_tensor(cams, 'cams', kernels).detach().double().contiguous()
    if tuple(cm.shape) != (V, CAM):
        raise ValueError(f'cams must be [{V}, {CAM}] (pack_cameras), got {list(cm.shape)}')
    return kp, cm, V, N, J


def triangulate(keypoints, cams, conf_min=CONF_MIN, tau_px=TAU_PX, min_angle_deg=MIN_ANGLE_DEG, min_views=MIN_VIEWS, refine=REFINE, rigid=None,
                want_undistorted=False):
    """`rohm_mv_triangulate`: keypoints [V,N,J,3] float32 (x, y in pixels as detected, confidence), cams [V,24] float64
    (`pack_cameras`), rigid [12] or [3,4] float64 or None (world -> output frame, R|t; None leaves the world frame), HIP tensors
    -> `Triangulation`.  One launch, no synchronisation, nothing read back; there is no CPU path."""
    kp, cm, V, N, J = views_operands(keypoints, cams, _TAKE)
    rg = None
    if rigid is not None:
        rg = _hip(rigid, 'rigid').detach().double()
        if tuple(rg.shape) == (3, 4):
            rg = torch.cat([rg[:, :3].reshape(9), rg[:, 3]])
        rg = rg.contiguous()
        if tuple(rg.shape) != (12,):
            raise ValueError(f'rigid must be [12] (R row-major, then t) or [3, 4], got {list(rigid.shape)}')
    dev = kp.device
    joints = torch.empty(N, J, 3, device=dev, dtype=torch.float64)
    conf = torch.empty(N, J, device=dev, dtype=torch.float32)
    report = torch.empty(N, J, 4, device=dev, dtype=torch.float64)
    inliers = torch.empty(N, J, device=dev, dtype=torch.int32)
    und = torch.empty(V, N, J, 3, device=dev, dtype=torch.float32) if want_undistorted else None
    with torch.cuda.device(dev):
        check(lib().rohm_mv_triangulate(ptr(kp), ptr(cm), ptr(rg), V, N, J, float(conf_min), float(tau_px), float(np.deg2rad(min_angle_deg)),
                                        int(min_views), int(refine), ptr(joints), ptr(conf), ptr(report), ptr(inliers), ptr(und),
                                        stream_ptr(dev)), 'rohm_mv_triangulate')
    return Triangulation(joints=joints, conf=conf, report=report, inliers=inliers, keypoints_und=und)


def view_residuals(joints_world, keypoints, cams, conf_min=CONF_MIN):
    """`rohm_mv_residuals`: joints_world [N,J,3] float64 in the world frame, keypoints and cams as `triangulate` (HIP tensors) ->
    resid [V,N,J] float64 on the device: the pixel distance between each detection as given and the joint projected with the
    forward distortion model, NaN where the view is unobserved, the joint is NaN or it lies behind the camera."""
    kp, cm, V, N, J = views_operands(keypoints, cams, _TAKE)
    jw = _hip(joints_world, 'joints_world').detach().double().contiguous()
    if tuple(jw.shape) != (N, J, 3):
        raise ValueError(f'joints_world must be [{N}, {J}, 3], got {list(jw.shape)}')
    resid = torch.empty(V, N, J, device=kp.device, dtype=torch.float64)
    with torch.cuda.device(kp.device):
        check(lib().rohm_mv_residuals(ptr(jw), ptr(kp), ptr(cm), V, N, J, float(conf_min), ptr(resid), stream_ptr(kp.device)), 'rohm_mv_residuals')
    return resid


# ---- host logic (float64 numpy) ---------------------------------------------------------------------------------------------------
def pack_cameras(camera_mtx, world2cam, dist_coeffs=None):
    """camera_mtx [V,3,3] (no skew), world2cam [V,4,4] (x_cam = R X + t), dist_coeffs [V,5] (k1 k2 p1 p2 k3) or None -> cams
    [V,24] float64: R (9, row-major), t (3), fx, fy, cx, cy, k1, k2, p1, p2, k3, three zeros."""
    K = np.asarray(camera_mtx, dtype=np.float64)
    W = np.asarray(world2cam, dtype=np.float64)
    if K.ndim != 3 or K.shape[1:] != (3, 3):
        raise ValueError(f'camera_mtx must be [V,3,3], got {K.shape}')
    V = K.shape[0]
    if W.shape != (V, 4, 4):
        raise ValueError(f'world2cam must be [{V},4,4], got {W.shape}')
    if not (np.isfinite(K).all() and np.isfinite(W).all()):
        raise ValueError('camera_mtx and world2cam must be finite')
    if (K[:, 0, 1] != 0).any() or (K[:, 1, 0] != 0).any() or (K[:, 2] != np.array([0.0, 0.0, 1.0])).any():
        raise ValueError('camera_mtx must be [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]: skew is not supported')
    if (K[:, 0, 0] <= 0).any() or (K[:, 1, 1] <= 0).any():
        raise ValueError('camera_mtx: focal lengths must be positive')
    cams = np.zeros((V, CAM))
    cams[:, :9] = W[:, :3, :3].reshape(V, 9)
    cams[:, 9:12] = W[:, :3, 3]
    cams[:, 12], cams[:, 13], cams[:, 14], cams[:, 15] = K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]
    if dist_coeffs is not None:
        D = np.asarray(dist_coeffs, dtype=np.float64)
        if D.shape != (V, 5) or not np.isfinite(D).all():
            raise ValueError(f'dist_coeffs must be [{V},5] and finite, got {D.shape}')
        cams[:, 16:21] = D
    return cams


def _read_time_key(d, N):
    """'fps' or 'times', whichever of the two a views file's dict gives, validated; `sync.frame_rate` reads it here too."""
    if ('fps' in d) == ('times' in d):
        raise ValueError('views: give exactly one of fps and times')
    if 'fps' in d:
        fps = np.asarray(d['fps'], dtype=np.float64)
        if fps.size != 1 or not np.isfinite(fps).all() or float(fps.reshape(-1)[0]) <= 0:
            raise ValueError(f'views: fps must be one positive number, got {d["fps"]!r}')
        return 'fps'
    times = np.asarray(d['times'], dtype=np.float64)
    if times.shape != (N,) or not np.isfinite(times).all() or (np.diff(times) <= 0).any():
        raise ValueError(f'views: times must be [{N}], finite and strictly increasing')
    return 'times'


def read_views(views, min_views=2):
    """Validate a views file (an .npz path or a dict) -> a dict with keypoints [V,N,K,3] float32 (K 22 or 25), camera_mtx
    [V,3,3], world2cam [V,4,4] (the inverse of cam2world where that was given), dist_coeffs [V,5] or None, world_up_axis 'z' |
    'y' | None, floor_height or None, and `time_key` ('fps' or 'times') with its value as given, frame_names and recording_name
    where given.  Required: keypoints_2d, camera_mtx, exactly one of world2cam and cam2world, exactly one of fps and times.  Any
    key outside `VIEW_KEYS` is refused by name.  `min_views`: the fewest views accepted (triangulation needs two; `rohm_amd.fit_views`
    reads a file with one)."""
    d = _lib.npz_dict(views)
    unknown = sorted(set(d) - set(VIEW_KEYS))
    if unknown:
        raise ValueError(f'views: unknown keys {unknown}; a views file has {list(VIEW_KEYS)}')
    missing = [k for k in ('keypoints_2d', 'camera_mtx') if k not in d]
    if missing:
        raise ValueError(f'views: missing {missing}')
    kp = np.asarray(d['keypoints_2d'], dtype=np.float32)
    if kp.ndim != 4 or kp.shape[1] < 1 or kp.shape[2:] not in ((22, 3), (25, 3)):
        raise ValueError(f'views: keypoints_2d must be [V,N,22,3] (SMPL order) or [V,N,25,3] (BODY_25) with N >= 1, got {kp.shape}')
    V, N = kp.shape[:2]
    if not min_views <= V <= 16:                                              # triangulation needs two; rohm_amd.fit_views reads one
        raise ValueError(f'views: the number of views must be in [{min_views}, 16], got {V}')
    if ('world2cam' in d) == ('cam2world' in d):
        raise ValueError('views: give exactly one of world2cam and cam2world')
    key = 'world2cam' if 'world2cam' in d else 'cam2world'
    W = np.asarray(d[key], dtype=np.float64)
    if W.shape != (V, 4, 4) or not np.isfinite(W).all():
        raise ValueError(f'views: {key} must be [{V},4,4] and finite, got {W.shape}')
    if key == 'cam2world':
        W = np.linalg.inv(W)
    K = np.asarray(d['camera_mtx'], dtype=np.float64)
    if K.shape != (V, 3, 3):
        raise ValueError(f'views: camera_mtx must be [{V},3,3], got {K.shape}')
    dist = None
    if 'dist_coeffs' in d:
        dist = np.asarray(d['dist_coeffs'], dtype=np.float64)
        if dist.shape != (V, 5):
            raise ValueError(f'views: dist_coeffs must be [{V},5], got {dist.shape}')
    try:
        pack_cameras(K, W, dist)
    except ValueError as e:
        raise ValueError(f'views: {e}') from None
    time_key = _read_time_key(d, N)
    up = None
    if 'world_up_axis' in d:
        up = str(np.asarray(d['world_up_axis']).reshape(-1)[0])
        if up not in ('z', 'y'):
            raise ValueError(f"views: world_up_axis must be 'z' or 'y', got {up!r}")
    floor = None
    if 'floor_height' in d:
        fh = np.asarray(d['floor_height'], dtype=np.float64)
        if fh.size != 1 or not np.isfinite(fh).all():
            raise ValueError(f'views: floor_height must be one finite number, got {d["floor_height"]!r}')
        if up is None:
            raise ValueError('views: floor_height needs world_up_axis (the axis the floor is perpendicular to)')
        floor = float(fh.reshape(-1)[0])
    if 'frame_names' in d and np.asarray(d['frame_names']).shape != (N,):
        raise ValueError(f'views: frame_names must be [{N}], got {np.asarray(d["frame_names"]).shape}')
    out = {'keypoints': np.ascontiguousarray(kp), 'camera_mtx': K, 'world2cam': W, 'dist_coeffs': dist, 'world_up_axis': up, 'floor_height': floor,
           'time_key': time_key}
    out[out['time_key']] = d[out['time_key']]
    out.update({k: d[k] for k in ('frame_names', 'recording_name') if k in d})
    return out


def _percentiles(x):
    x = x[np.isfinite(x)]
    return (float(np.median(x)), float(np.percentile(x, 95))) if x.size else (None, None)


def triangulate_views(views, ref_view=0, device='cuda:0', return_result=False, **options):
    """A views file (`read_views`) -> (skeleton dict, summary).  The skeleton has only `fit.SKELETON_KEYS` and
    `fit.PASS_THROUGH`: joints_3d [N,K,3] float32 in the camera frame of view `ref_view` (NaN where there is no result),
    joint_conf [N,K], fps or times as given, keypoints_2d (that view's undistorted keypoints), focal_length and camera_center
    (that view's; camera_mtx and dist_coeffs are not handed on: the keypoints are undistorted already and the track loader's
    undistortion mirrors x), frame_names and recording_name where given, and -- only when world_up_axis was given -- cam2world
    (the inverse of that view's world2cam), up_axis and floor_height.  `options` go to `triangulate`.  The summary counts the
    points with and without a result, the inlier counts, per view the share of its observed detections that were rejected and
    the median and 95th percentile of `view_residuals`, and the median sigma_m."""
    v = read_views(views)
    kp, W = v['keypoints'], v['world2cam']
    V, N, K = kp.shape[:3]
    if not 0 <= int(ref_view) < V:
        raise ValueError(f'ref_view must be in [0, {V}), got {ref_view}')
    ref = int(ref_view)
    device = torch.device(device)
    cams = pack_cameras(v['camera_mtx'], W, v['dist_coeffs'])
    rigid = np.concatenate([W[ref, :3, :3].reshape(9), W[ref, :3, 3]])
    kpd, camd, rgd = torch.from_numpy(kp).to(device), torch.from_numpy(cams).to(device), torch.from_numpy(rigid).to(device)
    conf_min = options.get('conf_min', CONF_MIN)
    tri = triangulate(kpd, camd, rigid=rgd, want_undistorted=True, **options)
    world = (tri.joints - rgd[9:]) @ rgd[:9].reshape(3, 3)                 # R^T (Y - t), row vectors
    resid = view_residuals(world, kpd, camd, conf_min=conf_min).cpu().numpy()
    joints, conf, report = tri.joints.cpu().numpy(), tri.conf.cpu().numpy(), tri.report.cpu().numpy()
    bits = tri.inliers.cpu().numpy().astype(np.int64)
    und = tri.keypoints_und.cpu().numpy()

    skeleton = {'joints_3d': joints.astype(np.float32), 'joint_conf': conf, v['time_key']: v[v['time_key']], 'keypoints_2d': und[ref],
                'focal_length': np.array([v['camera_mtx'][ref, 0, 0], v['camera_mtx'][ref, 1, 1]]),
                'camera_center': np.array([v['camera_mtx'][ref, 0, 2], v['camera_mtx'][ref, 1, 2]])}
    skeleton.update({k: v[k] for k in ('frame_names', 'recording_name') if k in v})
    if v['world_up_axis'] is not None:
        skeleton['cam2world'] = np.linalg.inv(W[ref])
        skeleton['up_axis'] = v['world_up_axis']
        if v['floor_height'] is not None:
            skeleton['floor_height'] = v['floor_height']

    has = report[..., 0] > 0
    with np.errstate(invalid='ignore'):
        seen = np.isfinite(kp).all(-1) & (kp[..., 2] > conf_min)              # [V,N,K], rule 1 on the host for the summary only
    per_view = []
    for i in range(V):
        used = ((bits >> i) & 1).astype(bool)
        n_seen = int((seen[i] & has).sum())
        med, p95 = _percentiles(resid[i])
        per_view.append({'view': i, 'observed': int(seen[i].sum()), 'rejected_share': (float((seen[i] & has & ~used).sum()) / n_seen) if n_seen else None,
                         'residual_median_px': med, 'residual_p95_px': p95})
    counts = report[..., 0].astype(np.int64)
    summary = {'views': V, 'frames': N, 'joints': K, 'ref_view': ref, 'points': int(has.size), 'triangulated': int(has.sum()),
               'without_result': int((~has).sum()), 'inlier_histogram': {str(k): int((counts == k).sum()) for k in range(V + 1) if (counts == k).any()},
               'per_view': per_view, 'median_sigma_m': float(np.median(report[..., 2][has])) if has.any() else None}
    return (skeleton, summary, tri) if return_result else (skeleton, summary)


# ---- the tool ------------------------------------------------------------------------------------------------------------------------
OPTIONS = (('tau_px', float, TAU_PX, 'a view is an inlier when it reprojects within this many pixels'),
           ('conf_min', float, CONF_MIN, 'a detection is observed when its confidence exceeds this'),
           ('min_angle_deg', float, MIN_ANGLE_DEG, 'a pair of views whose rays meet at less than this proposes nothing'),
           ('min_views', int, MIN_VIEWS, 'a point with fewer inliers has no result; 3 is recommended where four or more cameras see the person'),
           ('refine', int, REFINE, 'Gauss-Newton steps on the inliers\' reprojection error'))


def build_parser():
    ap = argparse.ArgumentParser(prog='python -m rohm_amd.multiview',
                                 description='triangulate the 2-D keypoints of several calibrated cameras and write a skeleton for rohm_amd.fit')
    ap.add_argument('--views', type=str, required=True, help='the views file (.npz): keypoints_2d, camera_mtx, world2cam or cam2world, fps or times')
    ap.add_argument('--out', type=str, required=True, help='write the skeleton here (.npz)')
    ap.add_argument('--ref_view', type=int, default=0, help='the skeleton is in this view\'s camera frame and carries its keypoints')
    for name, typ, default, text in OPTIONS:
        ap.add_argument('--' + name, type=typ, default=default, help=text + ' (chosen, not fitted)')
    ap.add_argument('--json', type=str, default='', help='write the summary and the per-point report here')
    ap.add_argument('--device', type=str, default='cuda:0')
    return ap


def _json_rows(a):
    return [[None if not np.isfinite(x) else float(x) for x in row] for row in np.asarray(a, dtype=np.float64).reshape(-1, a.shape[-1])]


def main(argv=None):
    args = build_parser().parse_args(argv)
    opts = {name: getattr(args, name) for name, _, _, _ in OPTIONS}
    try:
        skeleton, s, tri = triangulate_views(args.views, ref_view=args.ref_view, device=args.device, return_result=True, **opts)
    except (ValueError, _lib.RohmHipError) as e:
        raise SystemExit(f'{args.views}: {e}')
    print(' --------------- keypoints of %d views triangulated -------------' % s['views'])
    print('points triangulated / without result:  %d / %d of %d (%d frames x %d joints)' % (s['triangulated'], s['without_result'], s['points'],
                                                                                           s['frames'], s['joints']))
    print('inliers per point:                     ' + ', '.join('%s: %d' % kv for kv in s['inlier_histogram'].items()))
    for r in s['per_view']:
        fmt = (lambda x, f: '-' if x is None else f % x)
        print('view %2d: rejected %s of its observed detections, residual median / 95%% %s / %s px' % (
            r['view'], fmt(None if r['rejected_share'] is None else 100.0 * r['rejected_share'], '%.1f%%'), fmt(r['residual_median_px'], '%.2f'),
            fmt(r['residual_p95_px'], '%.2f')))
    print('median sigma_m:                        ' + ('-' if s['median_sigma_m'] is None else '%.2f mm per px' % (s['median_sigma_m'] * 1e3)))
    np.savez(args.out, **skeleton)
    print(f'[rohm_amd.multiview] wrote {args.out}' + ('' if 'cam2world' in skeleton else ' (no world_up_axis: python -m rohm_amd.floor finds the floor)'))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump({'views': args.views, 'summary': s, 'options': dict(opts, ref_view=args.ref_view),
                       'report': _json_rows(tri.report.cpu().numpy()), 'inliers': tri.inliers.cpu().numpy().reshape(-1).tolist()}, f, indent=1)
            f.write('\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
