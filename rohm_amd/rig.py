"""Calibrate a camera rig from the person's own 2-D keypoints: a views file without extrinsics to one with them.

`rohm_amd.multiview` and `rohm_amd.fit_views` take a calibrated rig.  Someone with three phones or four webcams round a room
has intrinsics (a checkerboard, the data sheet) and OpenPose files, and no `world2cam`.  The person who walks through the room is
the calibration target: every (frame, joint) seen by two views is a point correspondence.

    python -m rohm_amd.rig --views uncalibrated.npz --out views.npz --json report.json --body_model_path body_models/smplx_model
    python -m rohm_amd.multiview --views views.npz --out skeleton.npz          (or python -m rohm_amd.fit_views --views views.npz ...)

The rule (kernels in csrc/rig.hip, stated in full in include/rohm_rig.h, restated in tests/rig_ref.py).  All V (V - 1) / 2 pairs
of views go through one epipolar RANSAC call: `hypotheses` eight-point samples per pair, drawn here by a seeded generator from the
pair's common points, each solved for an essential matrix and scored by the number of common points within `tau_px` of Sampson
distance.  Each pair's winner is refitted `refits` times on its inliers, projected to singular values (1, 1, 0) and -- for the
edges of a maximum spanning tree over the inlier counts from `ref_view` -- decomposed; of the four (R, t) the one under which
`multiview.triangulate` places the most points in front of both cameras wins.  The tree chains the pairs, each edge's scale being
the median ratio of point distances over the points two triangulations share.  `multiview.triangulate` starts the points, and a
robust bundle adjustment (Levenberg-Marquardt on `fit_views`' energy, the points eliminated on the device, the cameras solved
here by Cholesky) refines cameras and points together.

Frame and scale.  The world is the reference camera's frame; `world_up_axis` is not written (`python -m rohm_amd.floor` finds the
floor later).  `--scale_from bones` (the default with a body model): the median over frames and bones of rest length over
triangulated length for the shins, forearms and upper arms; `baseline`: the distance from the reference camera to its first tree
neighbour is `--baseline_m`; `none`: that distance is 1.

`tau_px`, `sigma_px`, `hypotheses` and `min_inliers` are stated parameters: chosen on synthetic data, not fitted to recordings.

Limits: known intrinsics (and distortion); synchronised views (per-view time offsets are not estimated here: `python -m
rohm_amd.sync` first); one person; a static rig; a person who moves through the volume -- a person who stands still gives a
near-planar, near-degenerate cloud, which the
report shows as a low inlier share."""
from __future__ import annotations

import argparse
import ctypes as C
import functools
import json
import sys

import numpy as np
import torch

from . import _lib, multiview
from ._lib import check, lib, ptr, stream_ptr

CAM = multiview.CAM
N_MOM = 47
CONF_MIN, TAU_PX, SIGMA_PX, HYPOTHESES, REFITS, ITERS, MIN_INLIERS = 0.2, 4.0, 10.0, 1024, 2, 30, 50
LAMBDA0, LAMBDA_MIN, LAMBDA_MAX, TRIES = 1e-3, 1e-9, 1e8, 8
# SMPL joints: the shins, the forearms and the upper arms; BODY_25 has true counterparts for all of them
BONES = ((4, 7), (5, 8), (16, 18), (17, 19), (18, 20), (19, 21))
_TRI = [(i, j) for i in range(9) for j in range(i, 9)]
_TAKE = 'the rig kernels take'
_hip = functools.partial(_lib.hip_tensor, kernels=_TAKE)


# ---- the kernels' wrappers -----------------------------------------------------------------------------------------------------
def pair_ws_bytes(V, P):
    n = lib().rohm_rig_pair_ws_bytes(int(V), int(P))
    if n < 0:
        check(-1, 'rohm_rig_pair_ws_bytes')
    return int(n)


def ba_ws_bytes(V, P):
    n = lib().rohm_rig_ba_ws_bytes(int(V), int(P))
    if n < 0:
        check(-1, 'rohm_rig_ba_ws_bytes')
    return int(n)


def _workspace(nbytes, dev):
    return torch.empty((nbytes + 7) // 8, device=dev, dtype=torch.float64)


def _pairs(pairs):
    pr = _hip(pairs, 'pairs').detach().to(torch.int32).contiguous()
    if pr.dim() != 2 or pr.shape[1] != 2:
        raise ValueError(f'pairs must be [Q, 2], got {list(pr.shape)}')
    return pr, int(pr.shape[0])


def pair_hypotheses(keypoints, cams, pairs, samples, conf_min=CONF_MIN, tau_px=TAU_PX):
    """`rohm_rig_pair_hypotheses`: keypoints [V,N,J,3] float32, cams [V,24] float64 (the intrinsics are read), pairs [Q,2] int32,
    samples [Q,K,8] int32 (HIP tensors) -> E [Q,K,9] float64, counts [Q,K,2] int64 (inliers, common points), best [Q] int32.  Three
    launches, no synchronisation, nothing read back; there is no CPU path."""
    kp, cm, V, N, J = multiview.views_operands(keypoints, cams, _TAKE)
    pr, Q = _pairs(pairs)
    sm = _hip(samples, 'samples').detach().to(torch.int32).contiguous()
    if sm.dim() != 3 or sm.shape[0] != Q or sm.shape[2] != 8:
        raise ValueError(f'samples must be [{Q}, K, 8], got {list(sm.shape)}')
    K, dev = int(sm.shape[1]), kp.device
    E = torch.empty(Q, K, 9, device=dev, dtype=torch.float64)
    counts = torch.empty(Q, K, 2, device=dev, dtype=torch.int64)
    best = torch.empty(Q, device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        ws = _workspace(pair_ws_bytes(V, N * J), dev)
        check(lib().rohm_rig_pair_hypotheses(ptr(kp), ptr(cm), ptr(pr), ptr(sm), V, N, J, Q, K, float(conf_min), float(tau_px), ptr(ws), ptr(E),
                                             ptr(counts), ptr(best), stream_ptr(dev)), 'rohm_rig_pair_hypotheses')
    return E, counts, best


def pair_moments(keypoints, cams, pairs, E, conf_min=CONF_MIN, tau_px=TAU_PX):
    """`rohm_rig_pair_moments`: as above with E [Q,9] float64 -> moments [Q,47] float64: per pair the inliers' count, sum d^2 and
    the 45 upper-triangle sums of row^T row.  Two launches."""
    kp, cm, V, N, J = multiview.views_operands(keypoints, cams, _TAKE)
    pr, Q = _pairs(pairs)
    Ed = _lib.hip_rows(E, 'E', (Q, 9), _TAKE)
    out = torch.empty(Q, N_MOM, device=kp.device, dtype=torch.float64)
    with torch.cuda.device(kp.device):
        ws = _workspace(pair_ws_bytes(V, N * J), kp.device)
        check(lib().rohm_rig_pair_moments(ptr(kp), ptr(cm), ptr(pr), ptr(Ed), V, N, J, Q, float(conf_min), float(tau_px), ptr(ws), ptr(out),
                                          stream_ptr(kp.device)), 'rohm_rig_pair_moments')
    return out


def _points(points, N, J):
    X = _hip(points, 'points').detach().double().contiguous()
    if X.numel() != N * J * 3 or X.shape[-1] != 3:
        raise ValueError(f'points must be [{N * J}, 3] or [{N}, {J}, 3], got {list(X.shape)}')
    return X


def ba_moments(keypoints, cams, points, conf_min=CONF_MIN, sigma_px=SIGMA_PX, lam=LAMBDA0):
    """`rohm_rig_ba_moments`: cams [V,24] (the current rig), points [N J,3] float64 (NaN rows are outside the problem) -> S
    [6V,6V], r [6V], stats [2] = (E, the number of observations): the camera system of one Levenberg-Marquardt try with the points
    eliminated.  Two launches."""
    kp, cm, V, N, J = multiview.views_operands(keypoints, cams, _TAKE)
    X, dev = _points(points, N, J), kp.device
    S = torch.empty(6 * V, 6 * V, device=dev, dtype=torch.float64)
    r = torch.empty(6 * V, device=dev, dtype=torch.float64)
    stats = torch.empty(2, device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        ws = _workspace(ba_ws_bytes(V, N * J), dev)
        check(lib().rohm_rig_ba_moments(ptr(kp), ptr(cm), ptr(X), V, N, J, float(conf_min), float(sigma_px), float(lam), ptr(ws), ptr(S), ptr(r),
                                        ptr(stats), stream_ptr(dev)), 'rohm_rig_ba_moments')
    return S, r, stats


def ba_update(keypoints, cams, points, dc, conf_min=CONF_MIN, sigma_px=SIGMA_PX, lam=LAMBDA0):
    """`rohm_rig_ba_update`: the same operands and dc [V,6] float64 (delta omega, delta t per camera) -> points_new (the shape of
    `points`; a point outside the problem passes through), cams_new [V,24].  One launch."""
    kp, cm, V, N, J = multiview.views_operands(keypoints, cams, _TAKE)
    X, dev = _points(points, N, J), kp.device
    d = _lib.hip_rows(dc, 'dc', (V, 6), _TAKE)
    Xn, cn = torch.empty_like(X), torch.empty_like(cm)
    with torch.cuda.device(dev):
        check(lib().rohm_rig_ba_update(ptr(kp), ptr(cm), ptr(X), ptr(d), V, N, J, float(conf_min), float(sigma_px), float(lam), ptr(Xn), ptr(cn),
                                       stream_ptr(dev)), 'rohm_rig_ba_update')
    return Xn, cn


# ---- host logic (float64 numpy) ---------------------------------------------------------------------------------------------------
def _fix_sign(e):
    k = int(np.argmax(np.abs(e)))
    return -e if e[k] < 0 else e


def refit_from_moments(m):
    """A row of `pair_moments` -> the unit E [9] of the smallest eigenvalue of the inliers' 9 x 9 moment matrix (the sign rule of
    rohm_rig.h), or None with fewer than 8 inliers."""
    if not np.isfinite(m).all() or m[0] < 8:
        return None
    M = np.zeros((9, 9))
    for k, (i, j) in enumerate(_TRI):
        M[i, j] = M[j, i] = m[2 + k]
    return _fix_sign(np.linalg.eigh(M)[1][:, 0])


def decompose(E):
    """E [9] -> E projected to singular values (1, 1, 0) and its four (R, t), |t| = 1, for x2 = R x1 + t."""
    U, _, Vt = np.linalg.svd(np.asarray(E, dtype=np.float64).reshape(3, 3))
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    Wm = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    Ep = U @ np.diag([1.0, 1.0, 0.0]) @ Vt
    return Ep, [(U @ Wm @ Vt, U[:, 2]), (U @ Wm @ Vt, -U[:, 2]), (U @ Wm.T @ Vt, U[:, 2]), (U @ Wm.T @ Vt, -U[:, 2])]


def spanning_tree(weights, ref, min_inliers):
    """Prim's maximum spanning tree from `ref` over the symmetric [V,V] inlier counts, the lowest indices on ties -> [(parent,
    child)] in the order they join.  Edges below `min_inliers` do not exist; a view that cannot be reached is refused by name."""
    V = weights.shape[0]
    for v in range(V):
        if np.delete(weights[v], v).max() < min_inliers:
            raise ValueError(f'view {v}: every pair with it has fewer than min_inliers = {min_inliers} inliers (the most: '
                             f'{int(np.delete(weights[v], v).max())}); it shares too little of the walk with the other views')
    inside, edges = [ref], []
    while len(inside) < V:
        pick = None
        for a in sorted(inside):
            for b in range(V):
                if b not in inside and weights[a, b] >= min_inliers and (pick is None or weights[a, b] > weights[pick]):
                    pick = (a, b)
        if pick is None:
            left = sorted(set(range(V)) - set(inside))
            raise ValueError(f'views {left} cannot be chained to view {ref}: no pair between the two groups has min_inliers = {min_inliers} inliers')
        inside.append(pick[1])
        edges.append(pick)
    return edges


def _rigid(R, t):
    W = np.eye(4)
    W[:3, :3], W[:3, 3] = R, t
    return W


def _lm(kpd, cams, points, ref, sigma_px, iters, conf_min, log):
    """The Levenberg-Marquardt loop of rohm_rig.h over `ba_moments` / `ba_update` -> (cams, points, [E per iteration])."""
    V = cams.shape[0]
    keep = np.array([i for i in range(6 * V) if i // 6 != ref])
    lam = LAMBDA0
    S, r, stats = ba_moments(kpd, cams, points, conf_min, sigma_px, lam)
    E = float(stats[0])
    history = [E]
    if not np.isfinite(E):
        raise ValueError('the chained rig puts an observed point behind a camera: the pairwise geometry is inconsistent')
    for it in range(int(iters)):
        accepted = False
        for _ in range(TRIES):
            Sh, rh = S.cpu().numpy()[np.ix_(keep, keep)], r.cpu().numpy()[keep]
            ok = True
            try:
                L = np.linalg.cholesky(Sh)                                   # a pivot that is not positive rejects the try
            except np.linalg.LinAlgError:
                ok = False
            if ok:
                dc = np.zeros(6 * V)
                dc[keep] = -np.linalg.solve(L.T, np.linalg.solve(L, rh))
                Xt, ct = ba_update(kpd, cams, points, torch.from_numpy(dc.reshape(V, 6)).to(cams.device), conf_min, sigma_px, lam)
                lam_next = max(lam / 10.0, LAMBDA_MIN)
                St, rt, stt = ba_moments(kpd, ct, Xt, conf_min, sigma_px, lam_next)
                Et = float(stt[0])
                ok = Et < E                                                # an infinite (or NaN) energy is a rejected try
            if ok:
                gain = (E - Et) / E if E > 0 else 0.0
                cams, points, S, r, E, lam, accepted = ct, Xt, St, rt, Et, lam_next, True
                break
            lam = min(lam * 10.0, LAMBDA_MAX)
            S, r, _ = ba_moments(kpd, cams, points, conf_min, sigma_px, lam)
        history.append(E)
        if log:
            log(f'bundle adjustment {it + 1}: E = {E:.6g}, lambda = {lam:.1e}' + ('' if accepted else ' (no try accepted)'))
        if not accepted or gain < 1e-10:
            break
    return cams, points, history


def calibrate(keypoints, camera_mtx, dist_coeffs=None, ref_view=0, hypotheses=HYPOTHESES, tau_px=TAU_PX, refits=REFITS, sigma_px=SIGMA_PX,
              iters=ITERS, min_inliers=MIN_INLIERS, seed=0, conf_min=CONF_MIN, device='cuda:0', log=None):
    """keypoints [V,N,J,3] (x, y in pixels as detected, confidence), camera_mtx [V,3,3], dist_coeffs [V,5] or None -> (world2cam
    [V,4,4] float64 with the reference camera as the world and its first tree neighbour at distance 1, report dict).  The report:
    `pairs` (per pair the common points, the inliers, their share and the rms Sampson distance), `tree` ([(parent, child)]),
    `neighbour` (the first tree neighbour), `chained_world2cam` (before bundle adjustment), `energy` (E per iteration),
    `iterations`, `per_view` (the median and 95th percentile of `multiview.view_residuals`), `points` [N,J,3] (the adjusted points,
    NaN where there is none) and `triangulated`."""
    kp = np.ascontiguousarray(np.asarray(keypoints, dtype=np.float32))
    if kp.ndim != 4 or kp.shape[3] != 3:
        raise ValueError(f'keypoints must be [V,N,J,3], got {kp.shape}')
    V, N, J = kp.shape[:3]
    if not 2 <= V <= 16:
        raise ValueError(f'the number of views must be in [2, 16], got {V}')
    ref = int(ref_view)
    if not 0 <= ref < V:
        raise ValueError(f'ref_view must be in [0, {V}), got {ref_view}')
    if int(hypotheses) < 1 or int(refits) < 0 or int(iters) < 0 or int(min_inliers) < 8:
        raise ValueError(f'hypotheses must be >= 1, refits and iters >= 0 and min_inliers >= 8, got {hypotheses}, {refits}, {iters}, {min_inliers}')
    if not (np.isfinite(tau_px) and tau_px > 0 and np.isfinite(sigma_px) and sigma_px >= 0):
        raise ValueError(f'tau_px must be positive and sigma_px >= 0, got {tau_px}, {sigma_px}')
    eye = np.broadcast_to(np.eye(4), (V, 4, 4))
    cams0 = multiview.pack_cameras(camera_mtx, eye, dist_coeffs)
    device = torch.device(device)
    P, Kh = N * J, int(hypotheses)
    pairs = np.stack(np.triu_indices(V, 1), 1).astype(np.int32)
    Q = len(pairs)
    # step 1: the samples, drawn from each pair's common points (rule 1 on the host, for the drawing only)
    with np.errstate(invalid='ignore'):
        seen = (np.isfinite(kp).all(-1) & (kp[..., 2] > conf_min)).reshape(V, P)
    g = np.random.Generator(np.random.PCG64(int(seed)))
    samples = np.zeros((Q, Kh, 8), np.int32)
    n_common = np.zeros(Q, np.int64)
    for q, (v1, v2) in enumerate(pairs):
        idx = np.flatnonzero(seen[v1] & seen[v2])
        n_common[q] = len(idx)
        if len(idx) >= 8:
            samples[q] = idx[g.integers(0, len(idx), (Kh, 8))]             # a repeat within a sample makes that hypothesis degenerate
    if n_common.max() < 8:
        raise ValueError(f'no common points: no pair of views observes 8 points together (the most: {int(n_common.max())})')
    kpd, camd = torch.from_numpy(kp).to(device), torch.from_numpy(cams0).to(device)
    prd = torch.from_numpy(pairs).to(device)
    E_all, counts, best = pair_hypotheses(kpd, camd, prd, torch.from_numpy(samples).to(device), conf_min, tau_px)
    best_h = best.cpu().numpy()
    rows = torch.arange(Q, device=device)
    E = E_all[rows, best.clamp(min=0).long()].cpu().numpy()
    E[best_h < 0] = 0.0
    # step 2: the inlier refits
    mom = pair_moments(kpd, camd, prd, torch.from_numpy(E).to(device), conf_min, tau_px).cpu().numpy()
    for _ in range(int(refits)):
        for q in range(Q):
            e = refit_from_moments(mom[q])
            if e is not None:
                E[q] = e
        mom = pair_moments(kpd, camd, prd, torch.from_numpy(E).to(device), conf_min, tau_px).cpu().numpy()
    inl = np.where(np.isfinite(mom[:, 0]), mom[:, 0], 0).astype(np.int64)
    weights = np.zeros((V, V), np.int64)
    weights[pairs[:, 0], pairs[:, 1]] = weights[pairs[:, 1], pairs[:, 0]] = inl
    pair_report = [{'pair': [int(a), int(b)], 'common': int(n_common[q]), 'inliers': int(inl[q]),
                    'inlier_share': float(inl[q]) / int(n_common[q]) if n_common[q] else None,
                    'sampson_rms_px': float(np.sqrt(mom[q, 1] / inl[q])) if inl[q] else None} for q, (a, b) in enumerate(pairs)]
    # steps 3 to 6: the tree, each edge's (R, t) by cheirality, chained with its scale
    edges = spanning_tree(weights, ref, int(min_inliers))
    tri_tau = 2.5 * float(tau_px)
    W = {ref: np.eye(4)}
    cloud = {}                                                             # view -> (points [P,3] in the tree's world, has [P]) of its first edge
    for a, b in edges:
        v1, v2 = min(a, b), max(a, b)
        q = int(np.flatnonzero((pairs[:, 0] == v1) & (pairs[:, 1] == v2))[0])
        _, cands = decompose(E[q])
        two = torch.stack([kpd[v1], kpd[v2]])
        got = []
        for R, t in cands:
            c2 = cams0[[v1, v2]].copy()
            c2[1, :9], c2[1, 9:12] = R.reshape(9), t
            tr = multiview.triangulate(two, torch.from_numpy(c2).to(device), conf_min=conf_min, tau_px=tri_tau)
            got.append(tr.joints.reshape(P, 3).cpu().numpy())
        n_front = [int(np.isfinite(x).all(-1).sum()) for x in got]
        k = int(np.argmax(n_front))                                        # the most results; the first on ties
        if n_front[k] < 8:
            raise ValueError(f'views {v1} and {v2}: no decomposition of their essential matrix puts 8 points in front of both cameras')
        rel = _rigid(*cands[k])                                            # x_v2 = rel x_v1
        X1 = got[k]                                                        # in v1's frame, baseline 1
        if a == v2:                                                        # the parent is v2: the child's pose is the inverse
            rel = np.linalg.inv(rel)
            X1 = X1 @ cands[k][0].T + cands[k][1]                          # into the parent's frame
        has = np.isfinite(X1).all(-1)
        s = 1.0
        if a in cloud:                                                     # the scale of this edge against the tree's
            Xw, hw = cloud[a]
            both = has & hw
            if both.sum() < 3:
                raise ValueError(f'views {a} and {b}: their triangulation shares fewer than 3 points with the tree\'s; the scale of this edge is unknown')
            Xa = Xw[both] @ W[a][:3, :3].T + W[a][:3, 3]                   # the tree's points in the parent's frame
            s = float(np.median(np.linalg.norm(Xa, axis=-1) / np.linalg.norm(X1[both], axis=-1)))
        rel[:3, 3] *= s
        W[b] = rel @ W[a]
        Wa_inv = np.linalg.inv(W[a])
        Xworld = (s * X1) @ Wa_inv[:3, :3].T + Wa_inv[:3, 3]
        cloud.setdefault(a, (Xworld, has))
        cloud.setdefault(b, (Xworld, has))
    chained = np.stack([W[v] for v in range(V)])
    neighbour = edges[0][1]
    # steps 7 and 8: the points, then bundle adjustment
    cams = torch.from_numpy(multiview.pack_cameras(camera_mtx, chained, dist_coeffs)).to(device)
    tri = multiview.triangulate(kpd, cams, conf_min=conf_min, tau_px=tri_tau)
    n_start = int((tri.report[..., 0] > 0).sum())
    if n_start < 8:
        raise ValueError(f'only {n_start} points triangulate under the chained rig: nothing to adjust')
    cams, points, history = _lm(kpd, cams, tri.joints.reshape(P, 3), ref, float(sigma_px), int(iters), conf_min, log)
    cams_h = cams.cpu().numpy()
    world2cam = np.broadcast_to(np.eye(4), (V, 4, 4)).copy()
    world2cam[:, :3, :3], world2cam[:, :3, 3] = cams_h[:, :9].reshape(V, 3, 3), cams_h[:, 9:12]
    base = np.linalg.norm(world2cam[neighbour, :3, :3].T @ world2cam[neighbour, :3, 3])
    world2cam[:, :3, 3] /= base                                            # the baseline to the first neighbour is 1
    points = points / base
    cams = torch.from_numpy(multiview.pack_cameras(camera_mtx, world2cam, dist_coeffs)).to(device)
    # step 9: the report
    tri = multiview.triangulate(kpd, cams, conf_min=conf_min, tau_px=tri_tau)
    resid = multiview.view_residuals(tri.joints, kpd, cams, conf_min=conf_min).cpu().numpy()
    per_view = []
    for v in range(V):
        med, p95 = multiview._percentiles(resid[v])
        per_view.append({'view': v, 'residual_median_px': med, 'residual_p95_px': p95})
    report = {'views': V, 'frames': N, 'joints': J, 'ref_view': ref, 'pairs': pair_report, 'tree': [[int(a), int(b)] for a, b in edges],
              'neighbour': int(neighbour), 'chained_world2cam': chained, 'energy': history, 'iterations': len(history) - 1, 'per_view': per_view,
              'points': points.reshape(N, J, 3).cpu().numpy(), 'triangulated': int((tri.report[..., 0] > 0).sum()),
              'median_residual_px': multiview._percentiles(resid)[0]}
    return world2cam, report


# ---- scale -------------------------------------------------------------------------------------------------------------------------
def rest_bone_lengths(body_model, betas=None):
    """The lengths of `BONES` of the body model at `betas` (default the mean shape) and zero pose -> [6] float64."""
    from .data_loaders.dataloader_video import _body_model
    layer = _body_model(body_model, 'neutral', 'cpu')
    vt, sd, jr = (getattr(layer, k).detach().cpu().double().numpy() for k in ('v_template', 'shapedirs', 'J_regressor'))
    b = np.zeros(10) if betas is None else np.asarray(betas, dtype=np.float64).reshape(-1)[:10]
    joints = jr[:22] @ (vt + sd[:, :, :len(b)] @ b)
    return np.array([np.linalg.norm(joints[i] - joints[j]) for i, j in BONES])


def bone_scale(points, rest_lengths):
    """points [N,22,3] (SMPL order, NaN where there is none) -> the median over frames and bones of rest length / triangulated
    length."""
    ratios = [rest / np.linalg.norm(points[:, i] - points[:, j], axis=-1) for (i, j), rest in zip(BONES, rest_lengths)]
    r = np.concatenate(ratios)
    r = r[np.isfinite(r)]
    if not r.size:
        raise ValueError('scale_from bones: no frame has both ends of a shin, forearm or upper arm triangulated')
    return float(np.median(r))


def read_uncalibrated(views):
    """A views file without world2cam / cam2world -> `multiview.read_views`' dict (its validation, identity extrinsics stood in)."""
    d = _lib.npz_dict(views)
    given = [k for k in ('world2cam', 'cam2world') if k in d]
    if given:
        raise ValueError(f'views: {given[0]} is given: this rig is calibrated already (python -m rohm_amd.multiview takes it as it is)')
    if 'keypoints_2d' not in d:
        raise ValueError("views: missing ['keypoints_2d']")
    V = np.asarray(d['keypoints_2d']).shape[0] if np.asarray(d['keypoints_2d']).ndim else 0
    return multiview.read_views(dict(d, world2cam=np.broadcast_to(np.eye(4), (V, 4, 4))))


def calibrate_views(views, scale_from=None, baseline_m=None, body_model=None, betas=None, device='cuda:0', **options):
    """A views file without extrinsics -> (the same file's arrays with `world2cam` filled in: `multiview.read_views` takes it
    unchanged; report).  `scale_from`: 'bones' (the default when `body_model` is given), 'baseline' (needs `baseline_m`) or 'none'.
    `options` go to `calibrate`."""
    from .data_loaders.dataloader_video import OPENPOSE_TO_SMPL
    scale_from = scale_from or ('bones' if body_model is not None else 'none')
    if scale_from not in ('bones', 'baseline', 'none'):
        raise ValueError(f"scale_from must be 'bones', 'baseline' or 'none', got {scale_from!r}")
    if scale_from == 'bones' and body_model is None:
        raise ValueError('scale_from bones needs a body model (--body_model_path): the rest lengths of its bones set the scale')
    if scale_from == 'baseline' and not (baseline_m is not None and np.isfinite(baseline_m) and baseline_m > 0):
        raise ValueError(f'scale_from baseline needs a positive baseline_m, got {baseline_m!r}')
    v = read_uncalibrated(views)
    if v['world_up_axis'] is not None:
        raise ValueError('views: world_up_axis describes a world this file does not have yet: the world will be the reference camera (python -m '
                         'rohm_amd.floor finds the floor)')
    world2cam, report = calibrate(v['keypoints'], v['camera_mtx'], v['dist_coeffs'], device=device, **options)
    s = 1.0
    if scale_from == 'baseline':
        s = float(baseline_m)
    elif scale_from == 'bones':
        pts = report['points']
        if pts.shape[1] == 25:
            pts = pts[:, OPENPOSE_TO_SMPL[0:22]]
        s = bone_scale(pts, rest_bone_lengths(body_model, betas))
    world2cam = world2cam.copy()
    world2cam[:, :3, 3] *= s
    report['points'] = report['points'] * s
    report['scale_from'], report['scale'] = scale_from, s
    d = _lib.npz_dict(views)
    out = {k: d[k] for k in multiview.VIEW_KEYS if k in d}
    out['world2cam'] = world2cam
    return out, report


# ---- the tool ------------------------------------------------------------------------------------------------------------------------
OPTIONS = (('hypotheses', int, HYPOTHESES, 'eight-point samples per pair of views'),
           ('tau_px', float, TAU_PX, 'a common point is an inlier within this Sampson distance in pixels'),
           ('refits', int, REFITS, 'refits of each pair\'s winner on its inliers'),
           ('sigma_px', float, SIGMA_PX, 'scale of the robust function of the bundle adjustment in pixels; 0 is plain least squares'),
           ('iters', int, ITERS, 'Levenberg-Marquardt iterations of the bundle adjustment'),
           ('min_inliers', int, MIN_INLIERS, 'a pair with fewer inliers is no edge of the tree'))


def build_parser():
    ap = argparse.ArgumentParser(prog='python -m rohm_amd.rig',
                                 description='calibrate a static camera rig from the 2-D keypoints of a person who walks through it')
    ap.add_argument('--views', type=str, required=True, help='the views file (.npz) without world2cam / cam2world: keypoints_2d, camera_mtx, fps or times')
    ap.add_argument('--out', type=str, required=True, help='write the views file with world2cam here (.npz)')
    ap.add_argument('--json', type=str, default='', help='write the report here')
    ap.add_argument('--ref_view', type=int, default=0, help='this camera\'s frame is the world')
    for name, typ, default, text in OPTIONS:
        ap.add_argument('--' + name, type=typ, default=default, help=text + ' (chosen on synthetic data, not fitted)')
    ap.add_argument('--seed', type=int, default=0, help='of the generator that draws the samples')
    ap.add_argument('--scale_from', type=str, default='', choices=['', 'bones', 'baseline', 'none'], help='default: bones with a body model, else none')
    ap.add_argument('--baseline_m', type=float, default=None, help='the distance from the reference camera to its first tree neighbour')
    ap.add_argument('--body_model_path', type=str, default='')
    ap.add_argument('--betas', type=str, default='', help='a .npy or .npz (key betas) with the 10 shape coefficients; default the mean shape')
    ap.add_argument('--device', type=str, default='cuda:0')
    return ap


def _jsonable(x):
    if isinstance(x, dict):
        return {k: _jsonable(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_jsonable(v) for v in x]
    if isinstance(x, np.ndarray):
        return _jsonable(x.tolist())
    if isinstance(x, (float, np.floating)):
        return float(x) if np.isfinite(x) else None
    if isinstance(x, np.integer):
        return int(x)
    return x


def main(argv=None):
    args = build_parser().parse_args(argv)
    opts = {name: getattr(args, name) for name, _, _, _ in OPTIONS}
    betas = None
    if args.betas:
        loaded = np.load(args.betas, allow_pickle=False)
        betas = np.asarray(loaded['betas'] if hasattr(loaded, 'files') else loaded, dtype=np.float64).reshape(-1)
    try:
        out, rep = calibrate_views(args.views, scale_from=args.scale_from or None, baseline_m=args.baseline_m, body_model=args.body_model_path or None,
                                   betas=betas, device=args.device, ref_view=args.ref_view, seed=args.seed,
                                   log=lambda s: print('[rohm_amd.rig] ' + s), **opts)
    except (ValueError, _lib.RohmHipError) as e:
        raise SystemExit(f'{args.views}: {e}')
    print(' --------------- a rig of %d views calibrated from %d frames -------------' % (rep['views'], rep['frames']))
    for p in rep['pairs']:
        print('views %2d, %2d: %6d common points, %6d inliers (%s)' % (p['pair'][0], p['pair'][1], p['common'], p['inliers'],
                                                                      '-' if p['inlier_share'] is None else '%.1f%%' % (100.0 * p['inlier_share'])))
    print('tree from view %d: %s' % (rep['ref_view'], ', '.join('%d-%d' % tuple(e) for e in rep['tree'])))
    print('bundle adjustment: %d iterations, E %.6g -> %.6g' % (rep['iterations'], rep['energy'][0], rep['energy'][-1]))
    for r in rep['per_view']:
        print('view %2d: residual median / 95%% %s / %s px' % (r['view'], '-' if r['residual_median_px'] is None else '%.2f' % r['residual_median_px'],
                                                             '-' if r['residual_p95_px'] is None else '%.2f' % r['residual_p95_px']))
    print('scale from %s: %.6g' % (rep['scale_from'], rep['scale']))
    np.savez(args.out, **out)
    print(f'[rohm_amd.rig] wrote {args.out} (the world is camera {rep["ref_view"]}: python -m rohm_amd.floor finds the floor)')
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(_jsonable({'views': args.views, 'options': dict(opts, ref_view=args.ref_view, seed=args.seed),
                                 'report': {k: v for k, v in rep.items() if k != 'points'}}), f, indent=1)
            f.write('\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
