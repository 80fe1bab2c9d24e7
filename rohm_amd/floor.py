"""Find the floor of an uncalibrated track: gravity and height from feet.

A track (`rohm_amd.data_loaders.track`) needs a `cam2world` that puts the floor perpendicular to `up_axis`, and a
`floor_height` for the skating guidance, `use_scene_floor_height` and the floor columns of `rohm_amd.quality`.  Body
estimators give SMPL-X parameters in the camera frame and nothing else.  The information is in the track itself: a person
who walks leaves resting toes on one plane, and the rest of the body is on one side of it.

    python -m rohm_amd.floor --track raw.npz --body_model_path body_models/smplx_model --out calibrated.npz --json report.json

The rule (`estimate_floor`; kernels in csrc/floor.hip, stated in full in include/rohm_hip.h, restated in tests/floor_ref.py):
1. a toe position (joints 10, 11) is a contact candidate when its speed to the next valid frame is below `v_max`, that frame
   is at most `max_gap` away and, with keypoints, its confidence is above `conf_min` (`rohm_floor_candidates`);
2. RANSAC: `hypotheses` planes through random triples of candidates, each turned so that most joints are above it, scored
   as (candidates within `tau`) - (joints more than `under_tol` below it), all in one launch (`rohm_floor_hypotheses`);
3. `refine` least-squares steps: the plane through the inliers of the current plane, from their moments
   (`rohm_floor_moments`) and `numpy.linalg.eigh` of the 3 x 3 covariance on the host;
4. `cam2world` = the minimal rotation that takes the normal onto `up_axis`, and the translation that makes a world point's
   up coordinate its signed distance to the plane; `floor_height = -toe_height`.

Limits: a static camera (the speed gate works in the camera frame); one planar floor; the person must walk (contacts on one
spot or one line do not determine a normal: `min_extent`); the track is scaled in metres.  `toe_height` and the default
thresholds are chosen, not fitted to data: the fitted plane is the plane of resting toe *joints*, which sit a sole's
thickness above the ground, and the default 0.0 makes that plane the floor -- what the `pene` rule of `rohm_amd.quality`
assumes."""
from __future__ import annotations

import argparse
import functools
import json
import sys

import numpy as np
import torch

from . import _lib
from ._lib import UP_AXIS, check, lib, ptr, stream_ptr, up_index as _up

TOES = (10, 11)
N_MOMENTS = 11
ESTIMATE_FIELDS = ('normal', 'offset', 'cam2world', 'floor_height', 'candidates', 'support', 'under', 'rms', 'extent', 'hypothesis',
                   'tilt_deg', 'centroid', 'up_axis')


class FloorEstimate:
    """normal [3] and offset: the floor's plane n . p + d = 0 in the camera frame, n towards the body; cam2world [4,4] and
    floor_height (along up_axis, in the world cam2world makes); candidates: resting toe positions; support: those within
    tau of the plane; under: joints more than under_tol below the best RANSAC plane; rms of the supporters' distances (m);
    extent: the square root of the middle eigenvalue of their covariance (m) -- how far the contacts spread in their second
    direction; hypothesis: the best triple's index; tilt_deg: the angle between the camera's -y axis and n; centroid [3] of
    the supporters."""
    __slots__ = ESTIMATE_FIELDS

    def __init__(self, **kw):
        for k in ESTIMATE_FIELDS:
            setattr(self, k, kw[k])

    def as_dict(self):
        return {k: (getattr(self, k).tolist() if isinstance(getattr(self, k), np.ndarray) else getattr(self, k)) for k in ESTIMATE_FIELDS}

    def lines(self):
        n = self.normal
        return [' --------------- the floor of this track (camera frame) -------------',
                'normal:                      [%+.6f, %+.6f, %+.6f]' % tuple(n), 'offset (m):                  %+.6f' % self.offset,
                'tilt against camera -y (deg): %.3f' % self.tilt_deg,
                'contact candidates:          %d' % self.candidates,
                'support:                     %d (%.1f %%)' % (self.support, 100.0 * self.support / max(self.candidates, 1)),
                'joints under the floor:      %d' % self.under, 'rms of the supporters (mm):  %.2f' % (self.rms * 1000.0),
                'extent of the contacts (m):  %.3f' % self.extent, 'best hypothesis:             %d' % self.hypothesis,
                "up_axis / floor_height:      '%s' / %+.4f" % (self.up_axis, self.floor_height)]


# ---- host logic (float64 numpy; no device) ---------------------------------------------------------------------------------
def draw_triples(P, K, seed):
    """[K, 3] int32 indices into the P candidates: the same seed and the same track give the same hypotheses."""
    if P < 1 or K < 0:
        raise ValueError(f'draw_triples needs P >= 1 and K >= 0, got P={P} K={K}')
    return np.random.Generator(np.random.PCG64(seed)).integers(0, P, size=(K, 3)).astype(np.int32)


def plane_from_moments(m, origin, n_prev):
    """One least-squares step from `rohm_floor_moments`' sums m [11] about `origin` -> (n, d, centroid, eigenvalues
    ascending): n is the eigenvector of the covariance's smallest eigenvalue, signed to agree with n_prev."""
    m, origin = np.asarray(m, dtype=np.float64), np.asarray(origin, dtype=np.float64)
    cnt = m[0]
    mean = m[1:4] / cnt
    second = np.array([[m[4], m[5], m[6]], [m[5], m[7], m[8]], [m[6], m[8], m[9]]]) / cnt
    w, v = np.linalg.eigh(second - np.outer(mean, mean))
    n = v[:, 0]
    if float(n @ np.asarray(n_prev, dtype=np.float64)) < 0.0:
        n = -n
    centroid = origin + mean
    return n, -float(n @ centroid), centroid, w


def cam2world_from_plane(normal, offset, up_axis='z'):
    """[4,4]: R is the minimal rotation that takes the unit normal n onto the up unit vector e, R = I + [v]x + [v]x^2 /
    (1 + c) with v = n x e and c = n . e; for c < -1 + 1e-12 the half turn about e x x^ normalised (about e x y^ when
    |e x x^| < 0.5).  The translation is offset * e: the up coordinate of cam2world . p is n . p + offset."""
    n = np.asarray(normal, dtype=np.float64).reshape(3)
    e = np.zeros(3)
    e[_up(up_axis)] = 1.0
    c = float(n @ e)
    if c < -1.0 + 1e-12:
        a = np.cross(e, np.array([1.0, 0.0, 0.0]))
        if np.linalg.norm(a) < 0.5:
            a = np.cross(e, np.array([0.0, 1.0, 0.0]))
        a /= np.linalg.norm(a)
        R = 2.0 * np.outer(a, a) - np.eye(3)
    else:
        v = np.cross(n, e)
        vx = np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])
        R = np.eye(3) + vx + vx @ vx / (1.0 + c)
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = float(offset) * e
    return M


def plane_of_calibration(cam2world, up_axis='z', floor_height=0.0):
    """(n, d) in the camera frame of the plane a calibration calls the floor: the world points with up coordinate
    floor_height."""
    M = np.asarray(cam2world, dtype=np.float64).reshape(4, 4)
    k = _up(up_axis)
    return M[k, :3].copy(), float(M[k, 3]) - float(floor_height)


def make_estimate(normal, offset, up_axis, toe_height, candidates, m_final, origin, under, hypothesis):
    """The `FloorEstimate` of a final plane and the moments m_final [11] of its supporters about `origin`."""
    m = np.asarray(m_final, dtype=np.float64)
    support = int(m[0])
    if support > 0:
        _, _, centroid, w = plane_from_moments(m, origin, normal)
        rms, extent = float(np.sqrt(m[10] / m[0])), float(np.sqrt(max(w[1], 0.0)))
    else:
        centroid, rms, extent = np.full(3, np.nan), float('nan'), 0.0
    n = np.asarray(normal, dtype=np.float64).reshape(3)
    return FloorEstimate(normal=n, offset=float(offset), cam2world=cam2world_from_plane(n, offset, up_axis), floor_height=0.0 - float(toe_height),
                         candidates=int(candidates), support=support, under=int(under), rms=rms, extent=extent, hypothesis=int(hypothesis),
                         tilt_deg=float(np.degrees(np.arccos(np.clip(-n[1], -1.0, 1.0)))), centroid=centroid, up_axis=up_axis)


def check_candidates(candidates, min_candidates, strict):
    if candidates < 3:
        raise ValueError(f'{candidates} resting toe positions: a plane needs 3.  Nobody stands still in this track (v_max), or the toes are '
                         f'never confident (conf_min)')
    if strict and candidates < min_candidates:
        raise ValueError(f'only {candidates} resting toe positions, fewer than min_candidates={min_candidates}: too few contacts to trust a '
                         f'floor (strict=False / --force accepts it)')


def check_estimate(est, min_support=0.5, min_extent=0.10):
    """The refusals of a strict estimate: each names the number and the option."""
    ratio = est.support / max(est.candidates, 1)
    if ratio < min_support:
        raise ValueError(f'{est.support} of {est.candidates} contacts ({ratio:.2f}) lie within tau of the best plane, fewer than '
                         f'min_support={min_support}: there is no single floor in this track (strict=False / --force accepts it)')
    if est.extent < min_extent:
        raise ValueError(f'the contacts extend {est.extent:.3f} m in their second direction, less than min_extent={min_extent}: they are on '
                         f'one spot or one line and the normal is not determined -- a person who stands still cannot be calibrated '
                         f'(strict=False / --force accepts it)')


def compare_planes(est, cam2world, up_axis, floor_height=None):
    """(angle_deg between the given calibration's up direction and the estimated normal, height_diff: the height of the
    estimate's centroid above the given floor minus its height above the estimated one; None without floor_height)."""
    n_g, d_g = plane_of_calibration(cam2world, up_axis, 0.0 if floor_height is None else floor_height)
    n_g_len = np.linalg.norm(n_g)
    cos = float(n_g @ est.normal) / n_g_len
    angle = float(np.degrees(np.arctan2(np.linalg.norm(np.cross(n_g, est.normal)) / n_g_len, cos)))
    if floor_height is None:
        return angle, None
    given = float(n_g @ est.centroid) + d_g
    mine = float(est.normal @ est.centroid) + est.offset - est.floor_height
    return angle, given - mine


# ---- the kernels' wrappers -----------------------------------------------------------------------------------------------------
_hip = functools.partial(_lib.hip_tensor, kernels='the floor kernels take')


def floor_candidates(joints, times, valid_idx, keypoints=None, conf_min=0.2, v_max=0.10, max_gap=0.05):
    """`rohm_floor_candidates`: joints [N,22,3] float32, times [N] float64, valid_idx [Nv] int32, keypoints [N,22,3] float32
    or None (HIP tensors) -> flags [N,2] uint8."""
    j = _hip(joints, 'joints')
    if j.dim() != 3 or tuple(j.shape[1:]) != (22, 3):
        raise ValueError(f'joints must be [N, 22, 3], got {list(j.shape)}')
    N = int(j.shape[0])
    j = j.detach().float().contiguous()
    t = _hip(times, 'times').detach().double().contiguous()
    vi = _hip(valid_idx, 'valid_idx').detach().to(torch.int32).contiguous()
    if tuple(t.shape) != (N,) or vi.dim() != 1:
        raise ValueError(f'times must be [{N}] and valid_idx [Nv], got {list(t.shape)} {list(vi.shape)}')
    kp = None
    if keypoints is not None:
        kp = _hip(keypoints, 'keypoints').detach().float().contiguous()
        if tuple(kp.shape) != (N, 22, 3):
            raise ValueError(f'keypoints must be [{N}, 22, 3], got {list(kp.shape)}')
    flags = torch.empty(N, 2, device=j.device, dtype=torch.uint8)
    with torch.cuda.device(j.device):
        check(lib().rohm_floor_candidates(ptr(j), ptr(t), ptr(vi), ptr(kp), N, int(vi.shape[0]), float(conf_min), float(v_max),
                                          float(max_gap), ptr(flags), stream_ptr(j.device)), 'rohm_floor_candidates')
    return flags


def floor_hypotheses(points, joints, triples, tau=0.03, under_tol=0.08):
    """`rohm_floor_hypotheses`: points [P,3] float32, joints [NJ,3] float32, triples [K,3] int32 (HIP tensors) ->
    (planes [K,4] float64, scores [K,3] int64, best [1] int32) on the device."""
    p = _hip(points, 'points').detach().float().contiguous()
    q = _hip(joints, 'joints').detach().float().contiguous()
    tr = _hip(triples, 'triples').detach().to(torch.int32).contiguous()
    if p.dim() != 2 or p.shape[1] != 3 or q.dim() != 2 or q.shape[1] != 3 or tr.dim() != 2 or tr.shape[1] != 3:
        raise ValueError(f'points, joints and triples must be [P,3], [NJ,3] and [K,3]; got {list(p.shape)} {list(q.shape)} {list(tr.shape)}')
    K = int(tr.shape[0])
    planes = torch.empty(K, 4, device=p.device, dtype=torch.float64)
    scores = torch.empty(K, 3, device=p.device, dtype=torch.int64)
    best = torch.full((1,), -1, device=p.device, dtype=torch.int32)
    with torch.cuda.device(p.device):
        check(lib().rohm_floor_hypotheses(ptr(p), int(p.shape[0]), ptr(q), int(q.shape[0]), ptr(tr), K, float(tau), float(under_tol),
                                          ptr(planes), ptr(scores), ptr(best), stream_ptr(p.device)), 'rohm_floor_hypotheses')
    return planes, scores, best


def floor_moments(points, plane, origin, tau=0.03):
    """`rohm_floor_moments`: points [P,3] float32, plane [4] and origin [3] float64 (HIP tensors) -> out [11] float64 on
    the device."""
    p = _hip(points, 'points').detach().float().contiguous()
    if p.dim() != 2 or p.shape[1] != 3:
        raise ValueError(f'points must be [P,3], got {list(p.shape)}')
    pl = _hip(plane, 'plane').detach().double().contiguous()
    og = _hip(origin, 'origin').detach().double().contiguous()
    if pl.numel() != 4 or og.numel() != 3:
        raise ValueError(f'plane must be [4] and origin [3], got {list(pl.shape)} {list(og.shape)}')
    out = torch.zeros(N_MOMENTS, device=p.device, dtype=torch.float64)
    with torch.cuda.device(p.device):
        check(lib().rohm_floor_moments(ptr(p), int(p.shape[0]), ptr(pl), ptr(og), float(tau), ptr(out), stream_ptr(p.device)),
              'rohm_floor_moments')
    return out


# ---- the estimator -----------------------------------------------------------------------------------------------------------
def _host(x, dtype):
    return np.asarray(x.detach().cpu() if torch.is_tensor(x) else x).astype(dtype).reshape(-1)


def default_max_gap(times):
    """1.5 times the median interval, the rule of `data_loaders.track.default_max_gap`."""
    return float(1.5 * np.median(np.diff(times))) if len(times) > 1 else 0.0


def estimate_floor(joints, times=None, valid=None, keypoints=None, fps=30.0, up_axis='z', tau=0.03, under_tol=0.08, v_max=0.10,
                   max_gap=None, conf_min=0.2, hypotheses=4096, seed=0, refine=2, toe_height=0.0, min_candidates=30, min_support=0.5,
                   min_extent=0.10, strict=True):
    """The floor under a camera-frame track -> `FloorEstimate` (the rule: this module's docstring).  joints [N,22,3] float32
    HIP tensor in the camera frame, metres; times [N] seconds (default i / fps); valid [N] bool (default all); keypoints
    [N,22,3] (x, y, confidence, SMPL order; default: no confidence gate).  With `strict` a ValueError names the number and
    the option when there are fewer than min_candidates contacts, when fewer than min_support of them support the plane, or
    when they extend less than min_extent metres in their second direction.  There is no CPU path."""
    j = _hip(joints, 'joints')
    if j.dim() != 3 or tuple(j.shape[1:]) != (22, 3):
        raise ValueError(f'joints must be [N, 22, 3], got {list(j.shape)}')
    _up(up_axis)
    N, dev = int(j.shape[0]), j.device
    j = j.detach().float().contiguous()
    ts = np.arange(N, dtype=np.float64) / float(fps) if times is None else _host(times, np.float64)
    v = np.ones(N, bool) if valid is None else _host(valid, bool)
    if ts.shape != (N,) or v.shape != (N,):
        raise ValueError(f'times and valid must be [{N}], got {ts.shape} {v.shape}')
    if max_gap is None:
        max_gap = default_max_gap(ts)
    t_dev = torch.from_numpy(ts).to(dev)
    vi = torch.from_numpy(np.flatnonzero(v).astype(np.int32)).to(dev)
    flags = floor_candidates(j, t_dev, vi, keypoints, conf_min, v_max, max_gap)
    # compaction: plumbing, not arithmetic
    idx = torch.nonzero(flags.reshape(-1)).reshape(-1)
    points = j[:, TOES[0]:TOES[1] + 1].reshape(-1, 3).index_select(0, idx).contiguous()
    P = int(points.shape[0])
    check_candidates(P, min_candidates, strict)
    triples = draw_triples(P, int(hypotheses), seed)
    body = j.index_select(0, vi.long()).reshape(-1, 3).contiguous()
    planes, scores, best = floor_hypotheses(points, body, torch.from_numpy(triples).to(dev), tau, under_tol)
    h = int(best.cpu()[0])
    if h < 0:
        raise ValueError(f'all {int(hypotheses)} triples of contacts are degenerate (hypotheses={int(hypotheses)}): the contacts are on one line')
    plane = planes[h].cpu().numpy()
    under = int(scores[h, 2].cpu())
    origin = points.index_select(0, torch.from_numpy(triples[h].astype(np.int64)).to(dev)).cpu().numpy().astype(np.float64).mean(axis=0)
    og_dev = torch.from_numpy(origin).to(dev)
    n, d = plane[:3], float(plane[3])
    for _ in range(int(refine)):
        m = floor_moments(points, torch.from_numpy(np.append(n, d)).to(dev), og_dev, tau).cpu().numpy()
        if m[0] < 3:
            break
        n, d, _, _ = plane_from_moments(m, origin, n)
    m = floor_moments(points, torch.from_numpy(np.append(n, d)).to(dev), og_dev, tau).cpu().numpy()
    est = make_estimate(n, d, up_axis, toe_height, P, m, origin, under, h)
    if strict:
        check_estimate(est, min_support, min_extent)
    return est


def check_floor(joints_cam, cam2world, up_axis, floor_height=None, **kw):
    """Does a calibration meet the track's limit (the floor perpendicular to up_axis, at floor_height)?  ->
    (estimate, angle_deg, height_diff): `estimate_floor(joints_cam, up_axis=up_axis, **kw)` and `compare_planes` of it with
    the given calibration."""
    est = estimate_floor(joints_cam, up_axis=up_axis, **kw)
    angle, diff = compare_planes(est, cam2world, up_axis, floor_height)
    return est, angle, diff


def track_joints(track, body_model, device='cuda:0'):
    """(raw dict, `read_track`'s rec, joints [N,22,3] float32 in the camera frame on the device) of a track whose cam2world is
    optional: `read_track` validates a copy with a placeholder identity, so its refusals stay the single source of truth."""
    from .body_model import native_for
    from .data_loaders.dataloader_video import _body_model
    from .data_loaders.track import read_track
    from .export import _joints
    d = _lib.npz_dict(track)
    probe = dict(d)
    probe.setdefault('cam2world', np.eye(4))
    rec = read_track(probe)
    device = torch.device(device)
    body = _body_model(body_model, 'neutral', device)
    nat = native_for(body, device)
    p = {k: torch.from_numpy(np.ascontiguousarray(a)).to(nat.device) for k, a in rec['params'].items()}
    pose = torch.cat([p['global_orient'], p['body_pose']], dim=1).reshape(-1, 22, 3).contiguous()
    with torch.cuda.device(pose.device):
        joints = _joints(nat, pose, p['betas'].contiguous(), p['transl'].contiguous())
    return d, rec, joints


def calibrate_track(track, body_model, device='cuda:0', **kw):
    """Estimate the floor of a track (a path or a dict with the `TRACK_KEYS`; cam2world and floor_height are optional) ->
    (track dict, FloorEstimate).  The dict is the input plus cam2world, floor_height and up_axis -- no new key -- and is what
    `read_track` / `DataloaderTrack` / `drivers track` accept; `np.savez(path, **dict)` writes the file.  Joints come from
    `rohm_smplx_joints`; times, valid and the keypoints' confidences from the track; up_axis from `kw`, else the track's,
    else 'z'."""
    d, rec, joints = track_joints(track, body_model, device)
    up_axis = kw.pop('up_axis', None) or (rec['up_axis'] if 'up_axis' in d else 'z')
    kp = torch.from_numpy(rec['keypoints']).to(joints.device) if 'keypoints_2d' in d else None
    est = estimate_floor(joints, times=rec['times'], valid=rec['valid'], keypoints=kp, up_axis=up_axis, **kw)
    out = dict(d)
    out.update(cam2world=est.cam2world, floor_height=np.float64(est.floor_height), up_axis=np.array(up_axis))
    return out, est


# ---- the tool ------------------------------------------------------------------------------------------------------------------
OPTIONS = (('tau', float, 0.03, 'a contact within this distance (m) supports a plane'),
           ('under_tol', float, 0.08, 'a joint further than this (m) under a plane counts against it'),
           ('v_max', float, 0.10, 'a toe slower than this (m/s, camera frame) is at rest'),
           ('max_gap', float, None, 'the next frame must be at most this far away (s; default 1.5 median intervals)'),
           ('conf_min', float, 0.2, 'with keypoints_2d: a toe counts when its confidence is above this'),
           ('hypotheses', int, 4096, 'RANSAC planes'), ('seed', int, 0, 'seed of the triples'),
           ('toe_height', float, 0.0, 'height (m) of a resting toe joint above the ground; floor_height = -toe_height'))


def build_parser():
    ap = argparse.ArgumentParser(prog='python -m rohm_amd.floor',
                                 description='find the floor of an uncalibrated track: cam2world and floor_height from resting toes')
    ap.add_argument('--track', type=str, required=True, help='the track file (.npz); cam2world and floor_height may be missing')
    ap.add_argument('--body_model_path', type=str, default='body_models/smplx_model')
    ap.add_argument('--out', type=str, default='', help='write the calibrated track here (.npz)')
    ap.add_argument('--up_axis', choices=['z', 'y'], default=None, help="the world's up axis (default: the track's, else z)")
    for name, typ, default, text in OPTIONS:
        ap.add_argument('--' + name, type=typ, default=default, help=text)
    ap.add_argument('--force', action='store_true', help='strict=False: accept few contacts, weak support or a small extent')
    ap.add_argument('--json', type=str, default='', help='write the estimate here')
    ap.add_argument('--check', action='store_true', help="compare the track's own cam2world / floor_height with the estimate; writes no track")
    ap.add_argument('--device', type=str, default='cuda:0')
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    if not args.check and not args.out:
        raise SystemExit('give --out calibrated.npz (or --check)')
    kw = {name: getattr(args, name) for name, _, _, _ in OPTIONS}
    raw = _lib.npz_dict(args.track)
    if args.check and 'cam2world' not in raw:
        raise SystemExit(f'{args.track}: --check compares the track\'s cam2world with the estimate, and it has none')
    try:
        out, est = calibrate_track(raw, args.body_model_path, device=args.device, up_axis=args.up_axis, strict=not args.force, **kw)
    except ValueError as e:
        raise SystemExit(f'{args.track}: {e}')
    for line in est.lines():
        print(line)
    report = {'track': args.track, 'estimate': est.as_dict(), 'options': dict(kw, strict=not args.force)}
    if args.check:
        fh = float(np.asarray(raw['floor_height']).reshape(-1)[0]) if 'floor_height' in raw else None
        angle, diff = compare_planes(est, raw['cam2world'], est.up_axis, fh)
        report['check'] = {'angle_deg': angle, 'height_diff': diff}
        print('given cam2world against it:  %.6f deg%s' % (angle, '' if diff is None else ', floor %+.6f m' % diff))
    else:
        np.savez(args.out, **out)
        print(f'[rohm_amd.floor] wrote {args.out}')
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(report, f, indent=1)
            f.write('\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
