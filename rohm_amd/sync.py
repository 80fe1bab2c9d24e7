"""Synchronise a rig's cameras from the person: one constant time offset per view, estimated from the 2-D keypoints alone.

`rohm_amd.rig`, `rohm_amd.multiview` and `rohm_amd.fit_views` take synchronised views.  Three phones or four webcams round a room
are not hardware-triggered: their recordings start a few frames apart, and at walking speed one frame at 30 fps is some 3 cm of
body motion -- 8 px at 4 m with f = 1000 px, twice `rig`'s `tau_px`.  The person who walks through the room is the calibration
target already; they are the clock as well: under the right time shift the two views of a pair agree with ONE epipolar geometry,
under a wrong one the moving joints leave their epipolar lines.

    python -m rohm_amd.sync --views raw.npz --out synced.npz --json report.json
    python -m rohm_amd.rig --views synced.npz --out views.npz ...              (then rohm_amd.multiview / rohm_amd.fit_views)

The model (stated in full in include/provisional/rohm_sync.h, kernels in csrc/sync.hip, restated in tests/sync_ref.py).  All views
have N frames at one common, uniform rate: `fps`, or `times` uniform within 1e-6 relative; anything else is refused by name.
Frame n of view v was exposed at times[n] + offset_v, and offset_ref = 0.  For a pair (v1, v2) the shift s = (offset_v1 -
offset_v2) fps is in frames: view 1's frame n shows the instant of view 2's frame n + s.  Interpolation at a real frame index f:
i0 = floor(f), alpha = f - i0 in float64; alpha == 0 uses frame i0 alone, otherwise both brackets must lie in [0, N) and be usable
and the value is (1 - alpha) x(i0) + alpha x(i0 + 1).

The rule.  All V (V - 1) / 2 pairs.  With `world2cam` (a calibrated rig) each pair's E = [t]x R of its relative pose, one
`pair_sweep` over the integer shifts within +-ceil(max_offset_s fps) picks the shift of the smallest mean robust cost among those
with at least `min_inliers` common points, and one fine round follows.  Without it, for every integer shift one epipolar RANSAC
(`rig.pair_hypotheses`, `hypotheses` samples drawn by `rig`'s seeded host generator) runs on the two views sliced to their overlap
with its winner refitted twice on its inliers (`rig.pair_moments`; the count of the best of a few dozen random samples alone
is too noisy to tell two neighbouring shifts apart at 2 px of noise), and the coarse shift is the one with the largest inlier share
(the lowest |s| on ties); each of the `rounds` fine rounds then first resamples view 2 at the current estimate, fits E there in the
same way and sweeps.  A fine round is
one `pair_sweep` on est + k / 16, k = -16..16: the argmin of the mean robust cost, clamped to the interior, and the vertex of the
parabola through it and its two neighbours (a non-positive curvature keeps the grid point).  A pair is usable with at least
`min_inliers` inliers at its estimate; the offsets are the weighted least squares of s_ij = (o_i - o_j) fps over the usable pairs
(weights = inliers, o_ref = 0, Cholesky on the host); a view that no usable pair chains to the reference is refused by name.  The
output is the views file with every view's keypoints resampled (`rohm_sync_resample`, shifts[v] = -o_v fps) onto the reference
view's clock and every other key passed through: a valid views file with no key added.

`tau_px`, `sigma_px`, `hypotheses` and the 1/16 grid are stated parameters: chosen on synthetic data, not fitted to recordings.

Limits: constant offsets only -- drift, different frame rates, rolling shutter, more than one person and a moving rig are outside
the model; known intrinsics; a person who moves (a person who stands still is no clock: every shift costs the same, which the
report shows as a peak ratio near 1)."""
from __future__ import annotations

import argparse
import functools
import json
import math
import sys

import numpy as np
import torch

from . import _lib, multiview, rig
from ._lib import check, lib, ptr, stream_ptr

CAM = multiview.CAM
CONF_MIN, TAU_PX, SIGMA_PX, HYPOTHESES, ROUNDS, MIN_INLIERS, MAX_OFFSET_S = 0.2, 4.0, 4.0, 128, 3, 50, 1.0
GRID, HALF = 16, 16                                    # the fine sweep: est + k / GRID, k = -HALF..HALF
REFITS = 2
PAIRS_PER_CALL = 8                                     # two views per pair in a RANSAC call: the 16-view limit
UNIFORM_RTOL = 1e-6
_TAKE = 'the sync kernels take'
_hip = functools.partial(_lib.hip_tensor, kernels=_TAKE)


# ---- the kernels' wrappers -----------------------------------------------------------------------------------------------------
def ws_bytes(V, P):
    n = lib().rohm_sync_ws_bytes(int(V), int(P))
    if n < 0:
        check(-1, 'rohm_sync_ws_bytes')
    return int(n)


def pair_sweep(keypoints, cams, pairs, E, shifts, conf_min=CONF_MIN, tau_px=TAU_PX, sigma_px=SIGMA_PX):
    """`rohm_sync_pair_sweep`: keypoints [V,N,J,3] float32, cams [V,24] float64 (the intrinsics are read), pairs [Q,2] int32, E [Q,9]
    float64, shifts [Q,S] float64 in frames (HIP tensors) -> out [Q,S,4] float64: per (pair, shift) the common points, the inliers,
    sum d^2 / (d^2 + sigma_px^2) over the common points and sum d^2 over the inliers.  Two launches, no synchronisation, nothing read
    back; there is no CPU path."""
    kp, cm, V, N, J = multiview.views_operands(keypoints, cams, rig._TAKE)      # the views and the pairs are rig's operands, refused in rig's words
    pr, Q = rig._pairs(pairs)
    Ed = _lib.hip_rows(E, 'E', (Q, 9), _TAKE)
    sh = _hip(shifts, 'shifts').detach().double().contiguous()
    if sh.dim() != 2 or sh.shape[0] != Q or sh.shape[1] < 1:
        raise ValueError(f'shifts must be [{Q}, S] with S >= 1, got {list(sh.shape)}')
    S, dev = int(sh.shape[1]), kp.device
    out = torch.empty(Q, S, 4, device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        ws = torch.empty((ws_bytes(V, N * J) + 7) // 8, device=dev, dtype=torch.float64)
        check(lib().rohm_sync_pair_sweep(ptr(kp), ptr(cm), ptr(pr), ptr(Ed), ptr(sh), V, N, J, Q, S, float(conf_min), float(tau_px), float(sigma_px),
                                         ptr(ws), ptr(out), stream_ptr(dev)), 'rohm_sync_pair_sweep')
    return out


def resample_views(keypoints, shifts):
    """`rohm_sync_resample`: keypoints [V,N,J,3] float32, shifts [V] float64 in frames (HIP tensors) -> [V,N,J,3] float32: view v at
    the frame index n + shifts[v] (x, y linear in float64, the confidence the smaller of the two brackets', zeros outside the
    recording; a zero shift copies the bits).  One launch."""
    kp, V, N, J = multiview.keypoints_operand(keypoints, _TAKE)
    sh = _lib.hip_rows(shifts, 'shifts', (V,), _TAKE)
    out = torch.empty_like(kp)
    with torch.cuda.device(kp.device):
        check(lib().rohm_sync_resample(ptr(kp), ptr(sh), V, N, J, ptr(out), stream_ptr(kp.device)), 'rohm_sync_resample')
    return out


# ---- host logic (float64 numpy) ---------------------------------------------------------------------------------------------------
def essential(world2cam, v1, v2):
    """The unit E [9] (row-major, `rig`'s sign rule) with x2^T E x1 = 0 for the normalised coordinates of one point in the views v1
    and v2 of a calibrated rig: E = [t]x R for x_2 = R x_1 + t.  None when the two cameras share a centre."""
    W = np.asarray(world2cam, dtype=np.float64)
    R = W[v2, :3, :3] @ W[v1, :3, :3].T
    t = W[v2, :3, 3] - R @ W[v1, :3, 3]
    tx = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
    E = (tx @ R).reshape(9)
    n = np.linalg.norm(E)
    if not n > 1e-12 * max(1.0, np.linalg.norm(W[v1, :3, 3]), np.linalg.norm(W[v2, :3, 3])):
        return None
    return rig._fix_sign(E / n)


def solve_offsets(pairs, shifts, weights, V, ref=0):
    """pairs [Q,2], shifts [Q] (s_ij = o_i - o_j in frames), weights [Q] (0: the pair is not usable) -> (o [V] in frames with
    o[ref] = 0, residuals [Q] = s_ij - (o_i - o_j), NaN for an unusable pair): the weighted least squares, solved by Cholesky.  A view
    that no usable pair chains to `ref` is refused by name."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    s, w = np.asarray(shifts, dtype=np.float64).reshape(-1), np.asarray(weights, dtype=np.float64).reshape(-1)
    use = (w > 0) & np.isfinite(s)
    reached, grew = {int(ref)}, True
    while grew:
        grew = False
        for (a, b), u in zip(pairs, use):
            if u and ((int(a) in reached) != (int(b) in reached)):
                reached |= {int(a), int(b)}
                grew = True
    left = sorted(set(range(V)) - reached)
    if left:
        raise ValueError(f'views {left} cannot be chained to view {ref}: no usable pair (min_inliers inliers at its estimate) links the two groups; '
                         'they share too little of the walk with the other views')
    keep = [v for v in range(V) if v != ref]
    col = {v: k for k, v in enumerate(keep)}
    A, b = np.zeros((V - 1, V - 1)), np.zeros(V - 1)
    for (i, j), sq, wq, u in zip(pairs, s, w, use):
        if not u:
            continue
        row = np.zeros(V - 1)
        if int(i) != ref:
            row[col[int(i)]] = 1.0
        if int(j) != ref:
            row[col[int(j)]] = -1.0
        A += wq * np.outer(row, row)
        b += wq * sq * row
    o = np.zeros(V)
    if V > 1:
        L = np.linalg.cholesky(A)
        o[keep] = np.linalg.solve(L.T, np.linalg.solve(L, b))
    resid = np.where(use, s - (o[pairs[:, 0]] - o[pairs[:, 1]]), np.nan)
    return o, resid


def parabola_vertex(y_minus, y0, y_plus):
    """The offset in grid steps of the vertex of the parabola through (-1, y_minus), (0, y0), (1, y_plus), within [-1, 1]; 0 when the
    curvature is not positive or a value is not finite."""
    curv = y_minus - 2.0 * y0 + y_plus
    if not (np.isfinite(curv) and curv > 0.0):
        return 0.0
    return float(np.clip(0.5 * (y_minus - y_plus) / curv, -1.0, 1.0))


def _mean_cost(out, min_common):
    """out [Q,S,4] -> the mean robust cost [Q,S], +inf where fewer than `min_common` points are common (or the row is NaN)."""
    with np.errstate(all='ignore'):
        cost = out[..., 2] / out[..., 0]
    return np.where(np.isfinite(cost) & (out[..., 0] >= min_common), cost, np.inf)


def _first_best(values, shifts, largest):
    """The index of the best of `values`; among equal ones the lowest |shift|, then the lower shift."""
    v = np.asarray(values, dtype=np.float64)
    best = v.max() if largest else v.min()
    at = np.flatnonzero(v == best)
    return int(at[np.lexsort((shifts[at], np.abs(shifts[at])))[0]])


def _seen(kp, conf_min):
    with np.errstate(invalid='ignore'):
        return np.isfinite(kp).all(-1) & (kp[..., 2] > conf_min)


def _ransac(views1, views2, cams1, cams2, g, hypotheses, conf_min, tau_px, device, refits=0):
    """Epipolar RANSAC for the pairs (views1[k], views2[k]) (lists of [N',J,3] float32 arrays of one length, cams rows [24]),
    `PAIRS_PER_CALL` pairs per `rig.pair_hypotheses` call -> (E [Q,9] (zeros: no hypothesis), inliers [Q], common [Q])."""
    Q = len(views1)
    E, inl, com = np.zeros((Q, 9)), np.zeros(Q, np.int64), np.zeros(Q, np.int64)
    for lo in range(0, Q, PAIRS_PER_CALL):
        ks = list(range(lo, min(lo + PAIRS_PER_CALL, Q)))
        kp = np.ascontiguousarray(np.stack([views1[k] for k in ks] + [views2[k] for k in ks]))
        cm = np.stack([cams1[k] for k in ks] + [cams2[k] for k in ks])
        n = len(ks)
        pairs = np.stack([np.arange(n), n + np.arange(n)], 1).astype(np.int32)
        P = kp.shape[1] * kp.shape[2]
        seen = _seen(kp, conf_min).reshape(2 * n, P)
        samples = np.zeros((n, int(hypotheses), 8), np.int32)
        for k in range(n):
            idx = np.flatnonzero(seen[k] & seen[n + k])
            com[lo + k] = len(idx)
            if len(idx) >= 8:
                samples[k] = idx[g.integers(0, len(idx), (int(hypotheses), 8))]
        live = com[lo:lo + n] >= 8
        if not live.any():
            continue
        kpd, cmd, prd = torch.from_numpy(kp).to(device), torch.from_numpy(cm).to(device), torch.from_numpy(pairs).to(device)
        E_all, counts, best = rig.pair_hypotheses(kpd, cmd, prd, torch.from_numpy(samples).to(device), conf_min, tau_px)
        best_h, counts_h = best.cpu().numpy(), counts.cpu().numpy()
        rows = torch.arange(n, device=E_all.device)
        Eb = E_all[rows, best.clamp(min=0).long()].cpu().numpy()
        ok = live & (best_h >= 0)
        Eb[~ok] = 0.0
        got = np.where(ok, counts_h[np.arange(n), np.maximum(best_h, 0), 0], 0)
        for _ in range(int(refits)):
            mom = rig.pair_moments(kpd, cmd, prd, torch.from_numpy(Eb).to(device), conf_min, tau_px).cpu().numpy()
            for k in range(n):
                e = rig.refit_from_moments(mom[k]) if ok[k] else None
                if e is not None:
                    Eb[k] = e
        if refits:
            mom = rig.pair_moments(kpd, cmd, prd, torch.from_numpy(Eb).to(device), conf_min, tau_px).cpu().numpy()
            got = np.where(ok & np.isfinite(mom[:, 0]), mom[:, 0], 0).astype(np.int64)
        E[lo:lo + n], inl[lo:lo + n] = Eb, got
    return E, inl, com


def synchronise(keypoints, camera_mtx, dist_coeffs=None, fps=30.0, world2cam=None, ref_view=0, max_offset_s=MAX_OFFSET_S, tau_px=TAU_PX,
                sigma_px=SIGMA_PX, conf_min=CONF_MIN, hypotheses=HYPOTHESES, rounds=ROUNDS, min_inliers=MIN_INLIERS, seed=0, device='cuda:0',
                log=None):
    """keypoints [V,N,J,3] (x, y in pixels as detected, confidence), camera_mtx [V,3,3], dist_coeffs [V,5] or None, world2cam
    [V,4,4] or None (an uncalibrated rig) -> (keypoints [V,N,J,3] float32 on the clock of view `ref_view`, report).  The report:
    `offsets_s` and `offsets_frames` [V], `pairs` (per pair the coarse shift, the inlier share there and at the median shift and
    their ratio, the fine shift per round, the inliers at the estimate, whether it was usable and the cycle residual in frames) and
    `per_view` (the offset and the share of frames that fell outside the view's recording)."""
    kp = np.ascontiguousarray(np.asarray(keypoints, dtype=np.float32))
    if kp.ndim != 4 or kp.shape[3] != 3:
        raise ValueError(f'keypoints must be [V,N,J,3], got {kp.shape}')
    V, N, J = kp.shape[:3]
    if not 2 <= V <= 16:
        raise ValueError(f'the number of views must be in [2, 16], got {V}')
    ref = int(ref_view)
    if not 0 <= ref < V:
        raise ValueError(f'ref_view must be in [0, {V}), got {ref_view}')
    fps = float(fps)
    if not (np.isfinite(fps) and fps > 0):
        raise ValueError(f'fps must be positive, got {fps}')
    if not (np.isfinite(max_offset_s) and max_offset_s >= 0):
        raise ValueError(f'max_offset_s must be >= 0, got {max_offset_s}')
    if int(hypotheses) < 1 or int(rounds) < 1 or int(min_inliers) < 8:
        raise ValueError(f'hypotheses and rounds must be >= 1 and min_inliers >= 8, got {hypotheses}, {rounds}, {min_inliers}')
    if not (np.isfinite(tau_px) and tau_px > 0 and np.isfinite(sigma_px) and sigma_px >= 0):
        raise ValueError(f'tau_px must be positive and sigma_px >= 0, got {tau_px}, {sigma_px}')
    calibrated = world2cam is not None
    W = np.asarray(world2cam, dtype=np.float64) if calibrated else np.broadcast_to(np.eye(4), (V, 4, 4))
    cams = multiview.pack_cameras(camera_mtx, W, dist_coeffs)
    device = torch.device(device)
    pairs = np.stack(np.triu_indices(V, 1), 1).astype(np.int32)
    Q = len(pairs)
    M = min(int(math.ceil(float(max_offset_s) * fps)), N - 1)
    ints = np.arange(-M, M + 1, dtype=np.float64)
    kpd, camd, prd = torch.from_numpy(kp).to(device), torch.from_numpy(cams).to(device), torch.from_numpy(pairs).to(device)
    g = np.random.Generator(np.random.PCG64(int(seed)))
    sweep = functools.partial(pair_sweep, conf_min=conf_min, tau_px=tau_px, sigma_px=sigma_px)
    E = np.zeros((Q, 9))
    share = np.zeros((Q, len(ints)))                                       # the inlier share per integer shift
    # steps 2 and 3: E and the coarse shift per pair
    if calibrated:
        for q, (v1, v2) in enumerate(pairs):
            e = essential(W, v1, v2)
            E[q] = np.nan if e is None else e                              # two cameras at one place: no epipolar geometry, no inliers
        out = sweep(kpd, camd, prd, torch.from_numpy(E).to(device), torch.from_numpy(np.broadcast_to(ints, (Q, len(ints))).copy()).to(device))
        out = out.cpu().numpy()
        cost = _mean_cost(out, int(min_inliers))
        with np.errstate(all='ignore'):
            share = np.where(out[..., 0] > 0, out[..., 1] / out[..., 0], 0.0)
        coarse_at = np.array([_first_best(cost[q], ints, largest=False) for q in range(Q)])
        has_coarse = np.isfinite(cost[np.arange(Q), coarse_at])
    else:
        for k, s in enumerate(ints.astype(np.int64)):
            lo, hi = max(0, -s), min(N, N - s)                             # view 1's frames n with view 2's frame n + s inside
            _, inl, com = _ransac([kp[v1, lo:hi] for v1, _ in pairs], [kp[v2, lo + s:hi + s] for _, v2 in pairs], cams[pairs[:, 0]],
                                  cams[pairs[:, 1]], g, hypotheses, conf_min, tau_px, device, refits=REFITS)
            share[:, k] = np.where(com >= int(min_inliers), inl / np.maximum(com, 1), 0.0)
            if log:
                log(f'coarse shift {int(s):+d}: inlier shares ' + ' '.join('%.2f' % x for x in share[:, k]))
        coarse_at = np.array([_first_best(share[q], ints, largest=True) for q in range(Q)])
        has_coarse = share[np.arange(Q), coarse_at] > 0
    est = ints[coarse_at].copy()
    fine = [[] for _ in range(Q)]
    grid = np.arange(-HALF, HALF + 1, dtype=np.float64) / GRID
    # step 4: the fine rounds
    for r in range(1 if calibrated else int(rounds)):
        if not calibrated:
            v2s = kpd[torch.from_numpy(pairs[:, 1].astype(np.int64)).to(device)]
            moved = np.concatenate([resample_views(v2s[lo:lo + 16], torch.from_numpy(est[lo:lo + 16]).to(device)).cpu().numpy()
                                    for lo in range(0, Q, 16)])
            E, _, _ = _ransac([kp[v1] for v1, _ in pairs], list(moved), cams[pairs[:, 0]], cams[pairs[:, 1]], g, hypotheses, conf_min, tau_px,
                              device, refits=REFITS)
        shifts = est[:, None] + grid[None]
        out = sweep(kpd, camd, prd, torch.from_numpy(E).to(device), torch.from_numpy(shifts).to(device)).cpu().numpy()
        cost = _mean_cost(out, 8)
        for q in range(Q):
            if not (has_coarse[q] and np.isfinite(cost[q]).any()):
                fine[q].append(None)
                continue
            k = int(np.clip(_first_best(cost[q], grid, largest=False), 1, len(grid) - 2))
            est[q] = shifts[q, k] + parabola_vertex(cost[q, k - 1], cost[q, k], cost[q, k + 1]) / GRID
            fine[q].append(float(est[q]))
        if log:
            log(f'fine round {r + 1}: shifts ' + ' '.join('%+.3f' % x for x in est))
    # step 5: the offsets
    at = sweep(kpd, camd, prd, torch.from_numpy(E).to(device), torch.from_numpy(est[:, None].copy()).to(device)).cpu().numpy()[:, 0]
    inliers = np.where(np.isfinite(at[:, 1]) & has_coarse, at[:, 1], 0).astype(np.int64)
    usable = inliers >= int(min_inliers)
    o, resid = solve_offsets(pairs, est, np.where(usable, inliers, 0), V, ref)
    # step 6: every view on the reference view's clock
    synced = resample_views(kpd, torch.from_numpy(-o).to(device)).cpu().numpy()
    n_idx = np.arange(N, dtype=np.float64)
    per_view = []
    for v in range(V):
        f = n_idx - o[v]
        fl = np.floor(f)
        inside = (fl >= 0) & (fl < N) & ((f == fl) | (fl + 1 < N))
        per_view.append({'view': v, 'offset_s': float(o[v] / fps), 'offset_frames': float(o[v]), 'frames_outside_share': float(1.0 - inside.mean())})
    med = len(ints) // 2
    pair_report = []
    for q, (a, b) in enumerate(pairs):
        srt = np.sort(share[q])
        peak, median = float(share[q, coarse_at[q]]), float(srt[med])
        pair_report.append({'pair': [int(a), int(b)], 'coarse_shift': float(ints[coarse_at[q]]) if has_coarse[q] else None, 'inlier_share_at_coarse': peak,
                            'inlier_share_at_median_shift': median, 'peak_ratio': peak / median if median > 0 else None, 'fine_shifts': fine[q],
                            'shift_frames': float(est[q]), 'inliers': int(inliers[q]), 'usable': bool(usable[q]),
                            'cycle_residual_frames': float(resid[q]) if np.isfinite(resid[q]) else None})
    report = {'views': V, 'frames': N, 'joints': J, 'fps': fps, 'ref_view': ref, 'calibrated': bool(calibrated), 'max_shift_frames': M,
              'offsets_s': (o / fps).tolist(), 'offsets_frames': o.tolist(), 'pairs': pair_report, 'per_view': per_view}
    return synced, report


def frame_rate(d, N):
    """The common, uniform frame rate of a views file's arrays: `fps`, or `times` [N] uniform within 1e-6 relative; anything else
    is refused by name."""
    if multiview._read_time_key(d, N) == 'fps':
        return float(np.asarray(d['fps'], dtype=np.float64).reshape(-1)[0])
    times = np.asarray(d['times'], dtype=np.float64)
    if N < 2:
        raise ValueError('views: times of one frame give no frame rate; give fps')
    step = (times[-1] - times[0]) / (N - 1)
    worst = float(np.abs(np.diff(times) - step).max())
    if worst > UNIFORM_RTOL * step:
        raise ValueError(f'views: times is not uniform: a frame interval differs from the mean {step:.9g} s by {worst:.3g} s (more than {UNIFORM_RTOL:g} '
                         'relative); one constant offset per view needs one common, uniform rate (resample the detections first)')
    return 1.0 / step


def synchronise_views(views, device='cuda:0', **options):
    """A views file (an .npz path or a dict) with or without world2cam / cam2world -> (the same file's arrays with `keypoints_2d`
    resampled onto the reference view's clock -- no key added, every other key passed through --, report).  `options` go to
    `synchronise`."""
    d = _lib.npz_dict(views)
    if 'keypoints_2d' not in d:
        raise ValueError("views: missing ['keypoints_2d']")
    shape = np.asarray(d['keypoints_2d']).shape
    if len(shape) == 4 and shape[0] < 2:
        raise ValueError(f'views: the number of views must be in [2, 16], got {shape[0]}: one view has nothing to be synchronised with')
    calibrated = 'world2cam' in d or 'cam2world' in d
    V = shape[0] if len(shape) else 0
    v = multiview.read_views(d if calibrated else dict(d, world2cam=np.broadcast_to(np.eye(4), (V, 4, 4))))      # unknown keys are refused here
    fps = frame_rate(d, v['keypoints'].shape[1])
    synced, report = synchronise(v['keypoints'], v['camera_mtx'], v['dist_coeffs'], fps, v['world2cam'] if calibrated else None, device=device,
                                 **options)
    out = {k: d[k] for k in multiview.VIEW_KEYS if k in d}
    out['keypoints_2d'] = synced
    return out, report


# ---- the tool ------------------------------------------------------------------------------------------------------------------------
OPTIONS = (('max_offset_s', float, MAX_OFFSET_S, 'the largest time offset between two views that is searched, in seconds'),
           ('tau_px', float, TAU_PX, 'a common point is an inlier within this Sampson distance in pixels'),
           ('sigma_px', float, SIGMA_PX, 'scale of the robust cost of the sweeps in pixels; 0 is the plain sum of squares'),
           ('conf_min', float, CONF_MIN, 'a detection is observed above this confidence'),
           ('hypotheses', int, HYPOTHESES, 'eight-point samples per pair of views and shift (an uncalibrated rig)'),
           ('rounds', int, ROUNDS, 'alternations of refit and fine sweep (an uncalibrated rig; a calibrated one takes one)'),
           ('min_inliers', int, MIN_INLIERS, 'a pair with fewer inliers at its estimate does not vote'))


def build_parser():
    ap = argparse.ArgumentParser(prog='python -m rohm_amd.sync',
                                 description='estimate one constant time offset per camera from the 2-D keypoints of a person who walks through the '
                                             'rig, and resample every view onto the reference view\'s clock')
    ap.add_argument('--views', type=str, required=True, help='the views file (.npz), with or without world2cam / cam2world')
    ap.add_argument('--out', type=str, required=True, help='write the synchronised views file here (.npz): the same keys')
    ap.add_argument('--json', type=str, default='', help='write the offsets and the diagnostics here')
    ap.add_argument('--ref_view', type=int, default=0, help='this view\'s clock is kept')
    for name, typ, default, text in OPTIONS:
        ap.add_argument('--' + name, type=typ, default=default, help=text + ' (a stated parameter, chosen on synthetic data)')
    ap.add_argument('--seed', type=int, default=0, help='of the generator that draws the samples')
    ap.add_argument('--device', type=str, default='cuda:0')
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    opts = {name: getattr(args, name) for name, _, _, _ in OPTIONS}
    try:
        out, rep = synchronise_views(args.views, device=args.device, ref_view=args.ref_view, seed=args.seed,
                                     log=lambda s: print('[rohm_amd.sync] ' + s), **opts)
    except (ValueError, _lib.RohmHipError) as e:
        raise SystemExit(f'{args.views}: {e}')
    print(' --------------- %d views of %d frames synchronised (%s rig) -------------' % (rep['views'], rep['frames'],
                                                                                        'a calibrated' if rep['calibrated'] else 'an uncalibrated'))
    for p in rep['pairs']:
        print('views %2d, %2d: shift %+8.3f frames (coarse %s), %6d inliers%s, peak ratio %s' % (
            p['pair'][0], p['pair'][1], p['shift_frames'], '-' if p['coarse_shift'] is None else '%+d' % p['coarse_shift'], p['inliers'],
            '' if p['usable'] else ' (not usable)', '-' if p['peak_ratio'] is None else '%.1f' % p['peak_ratio']))
    for r in rep['per_view']:
        print('view %2d: offset %+9.4f s (%+8.3f frames), %.1f%% of its frames outside the recording' % (r['view'], r['offset_s'], r['offset_frames'],
                                                                                                      100.0 * r['frames_outside_share']))
    np.savez(args.out, **out)
    print(f'[rohm_amd.sync] wrote {args.out} (on the clock of view {rep["ref_view"]}; python -m rohm_amd.rig or rohm_amd.multiview take it as it is)')
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(rig._jsonable({'views': args.views, 'options': dict(opts, ref_view=args.ref_view, seed=args.seed), 'report': rep}), f, indent=1)
            f.write('\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
