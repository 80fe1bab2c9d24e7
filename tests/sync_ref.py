"""TEST INFRASTRUCTURE ONLY: float64 numpy restatement of csrc/sync.hip (`rohm_sync_pair_sweep`, `rohm_sync_resample`), the rule
the kernels are held to in tests/test_gpu_sync.py, itself held to tests/rig_ref.py's `pair_moments`, to closed forms and to the
recovery of planted offsets in tests/test_sync_ref.py.  The rule is stated in include/provisional/rohm_sync.h.  Inputs are taken as
float32 where the kernels read float32 and every operation is float64; the sums over points are numpy's.

Besides the kernel's output `pair_sweep` returns two margins per (pair, shift) on which the equalities of the GPU tests rest:
`margin_tau`, the least |d - tau_px| over the common points, and `margin_index`, the least distance of an interpolation index n + s
from an integer (infinite for a shift that is an integer exactly: alpha == 0 is then exact in float64 for every n).

`torch_*` wrap the two with the signatures of `rohm_amd.sync`'s kernel wrappers on CPU tensors, so that a test without a GPU can
run `sync.synchronise` on them (with tests/rig_ref.py under `rohm_amd.rig`).

The body is a smooth-in-time walker of its own (`walker`): `rig_ref.walking_body`'s sway is white noise per frame, which cannot be
interpolated between frames."""
import numpy as np

import helpers
import multiview_ref as MR
import rig_ref as RR

record = helpers.parity_recorder('sync_parity.json')
FPS = 30.0


# ---- rohm_sync_pair_sweep ---------------------------------------------------------------------------------------------------------
def brackets(N, shift):
    """The interpolation of every frame n at f = n + shift -> (i0 [N] int64 clipped into [0, N), alpha [N], exists [N]: alpha == 0 and
    i0 inside, or both brackets inside)."""
    f = np.arange(N, dtype=np.float64) + np.float64(shift)
    fl = np.floor(f)
    alpha = f - fl
    inside = (fl >= 0) & (fl < N)
    exists = inside & ((alpha == 0.0) | (fl + 1 < N))
    return np.clip(fl, 0, N - 1).astype(np.int64), alpha, exists


def pair_sweep(keypoints, cams, pairs, E, shifts, conf_min=0.2, tau_px=4.0, sigma_px=4.0, with_margins=False):
    """-> out [Q,S,4]: the common points, the inliers, sum d^2 / (d^2 + sigma_px^2) over the common points (sum d^2 at sigma_px = 0),
    sum d^2 over the inliers; a row of NaN for a pair outside [0, V) or with v1 = v2 and for a shift that is not finite."""
    cams = np.asarray(cams, dtype=np.float64)
    pairs = np.asarray(pairs).reshape(-1, 2)
    E = np.asarray(E, dtype=np.float64).reshape(-1, 9)
    shifts = np.asarray(shifts, dtype=np.float64)
    V, N, J = np.asarray(keypoints).shape[:3]
    ab = RR.undistorted(keypoints, cams, conf_min).reshape(V, N, J, 2)
    Q, S = shifts.shape
    out = np.full((Q, S, 4), np.nan)
    margin_tau = np.full((Q, S), np.inf)
    margin_index = np.full((Q, S), np.inf)
    for q, (v1, v2) in enumerate(pairs):
        if not (0 <= v1 < V and 0 <= v2 < V) or v1 == v2:
            continue
        scale = RR.pair_scale(cams, v1, v2)
        for s in range(S):
            if not np.isfinite(shifts[q, s]):
                continue
            i0, alpha, exists = brackets(N, shifts[q, s])
            i1 = np.minimum(i0 + 1, N - 1)
            al = alpha[:, None, None]
            with np.errstate(invalid='ignore'):
                x2 = np.where(al == 0.0, ab[v2][i0], (1.0 - al) * ab[v2][i0] + al * ab[v2][i1])
            common = exists[:, None] & np.isfinite(ab[v1]).all(-1) & np.isfinite(x2).all(-1)
            d = RR.sampson(E[q], ab[v1][common], x2[common], scale)
            fin = np.isfinite(d) & np.isfinite(d * d)
            with np.errstate(invalid='ignore'):
                inl = fin & (d <= tau_px)
            d2 = d[fin] ** 2
            sup = 1.0 if sigma_px > 0.0 else np.inf
            robust = (d2 / (d2 + sigma_px * sigma_px)).sum() if sigma_px > 0.0 else d2.sum()
            if (~fin).any():
                robust = robust + sup * (~fin).sum()
            out[q, s] = (common.sum(), inl.sum(), robust if common.any() else 0.0, (d[inl] ** 2).sum())
            if fin.any():
                margin_tau[q, s] = np.abs(d[fin] - tau_px).min()
            frac = alpha[exists & (alpha != 0.0)] if shifts[q, s] != np.floor(shifts[q, s]) else np.zeros(0)
            if frac.size:
                margin_index[q, s] = np.minimum(frac, 1.0 - frac).min()
    return (out, margin_tau, margin_index) if with_margins else out


# ---- rohm_sync_resample -----------------------------------------------------------------------------------------------------------
def resample(keypoints, shifts):
    """-> [V,N,J,3] float32: view v at the frame index n + shifts[v] by the rule of rohm_sync.h."""
    kp = np.ascontiguousarray(np.asarray(keypoints, dtype=np.float32))
    V, N, J = kp.shape[:3]
    shifts = np.asarray(shifts, dtype=np.float64).reshape(V)
    out = np.zeros_like(kp)
    for v in range(V):
        if not np.isfinite(shifts[v]):
            continue
        i0, alpha, exists = brackets(N, shifts[v])
        i1 = np.minimum(i0 + 1, N - 1)
        a, b = kp[v][i0], kp[v][i1]                                        # [N,J,3]
        with np.errstate(invalid='ignore'):
            ha = np.isfinite(a).all(-1) & (a[..., 2] > 0)
            hb = np.isfinite(b).all(-1) & (b[..., 2] > 0)
            al = alpha[:, None, None]
            xy = ((1.0 - al) * a[..., :2].astype(np.float64) + al * b[..., :2].astype(np.float64)).astype(np.float32)
            both = np.concatenate([xy, np.minimum(a[..., 2:], b[..., 2:])], -1)
        zero = np.zeros(3, np.float32)
        only_a = np.concatenate([a[..., :2], np.zeros_like(a[..., 2:])], -1)
        only_b = np.concatenate([b[..., :2], np.zeros_like(b[..., 2:])], -1)
        mixed = np.where((ha & hb)[..., None], both, np.where(ha[..., None], only_a, np.where(hb[..., None], only_b, zero)))
        res = np.where(exists[:, None, None], mixed, zero)
        exact = exists & (alpha == 0.0)
        res.view(np.uint32)[exact] = a.view(np.uint32)[exact]              # the frame itself, bit for bit
        out[v] = res
    return out


# ---- the two as `rohm_amd.sync`'s kernel wrappers on CPU tensors -----------------------------------------------------------------------
def torch_pair_sweep(keypoints, cams, pairs, E, shifts, conf_min=0.2, tau_px=4.0, sigma_px=4.0):
    import torch
    return torch.from_numpy(pair_sweep(keypoints.numpy(), cams.numpy(), pairs.numpy(), E.numpy(), shifts.numpy(), conf_min, tau_px, sigma_px))


def torch_resample_views(keypoints, shifts):
    import torch
    return torch.from_numpy(resample(keypoints.numpy(), shifts.numpy()))


def on_reference(monkeypatch):
    """Put the restatements under `rohm_amd.sync`, `rohm_amd.rig` and `rohm_amd.multiview`: the host logic then runs without a GPU."""
    from rohm_amd import sync
    RR.on_reference(monkeypatch)
    monkeypatch.setattr(sync, 'pair_sweep', torch_pair_sweep)
    monkeypatch.setattr(sync, 'resample_views', torch_resample_views)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def walker(times, J, seed, radius=1.2, centre=(0.0, 0.0, 1.0), speed=1.3):
    """A J-point "body" (a cloud some 0.5 x 0.3 x 1.7 m) at the instants `times` [M] in seconds -> X [M,J,3].  It walks a circle of
    `radius` at `speed` m/s and turns with it; every point swings about its place with two sinusoids of its own (0.7 to 1.8 Hz, up to
    8 cm: limb accelerations of up to 10 m/s^2): smooth in time, so that a detection between two frames is close to the line between them."""
    g = np.random.Generator(np.random.PCG64(seed))
    t = np.asarray(times, dtype=np.float64)
    body = g.uniform(-1.0, 1.0, (J, 3)) * np.array([0.25, 0.15, 0.85])
    amp = g.uniform(0.02, 0.08, (2, J, 3))
    freq = g.uniform(0.7, 1.8, (2, J, 3))
    phase = g.uniform(0.0, 2.0 * np.pi, (2, J, 3))
    sway = (amp[None] * np.sin(2.0 * np.pi * freq[None] * t[:, None, None, None] + phase[None])).sum(1)      # [M,J,3]
    phi = speed / radius * t + g.uniform(0, 2 * np.pi)
    c, s = np.cos(phi), np.sin(phi)
    Rz = np.stack([np.stack([-s, -c, 0 * c], -1), np.stack([c, -s, 0 * c], -1), np.stack([0 * c, 0 * c, 1 + 0 * c], -1)], -2)
    X = np.einsum('nij,nkj->nki', Rz, body[None] + sway)
    return X + np.array(centre) + radius * np.stack([c, s, 0 * c], -1)[:, None]


def make_scene(V, N, J, seed, offsets_frames, noise_px=0.0, distortion=True, fps=FPS):
    """-> (camera_mtx, world2cam, dist, keypoints [V,N,J,3] float32): `MR.make_rig` cameras that see the walker; frame n of view v
    shows the instant (n + offsets_frames[v]) / fps."""
    K, W, D = MR.make_rig(V, seed, distortion)
    from rohm_amd.multiview import pack_cameras
    cams = pack_cameras(K, W, D)
    g = np.random.Generator(np.random.PCG64(seed + 2))
    kp = np.zeros((V, N, J, 3), np.float32)
    for v in range(V):
        X = walker((np.arange(N) + float(offsets_frames[v])) / fps, J, seed + 1)
        px, depth = MR.project(cams[v:v + 1], X.reshape(-1, 3))
        assert (depth > 0.5).all()
        px = px[0] + g.standard_normal(px[0].shape) * noise_px
        kp[v] = np.concatenate([px, g.uniform(0.5, 1.0, (N * J, 1))], -1).reshape(N, J, 3)
    return K, W, D, kp


def pair_shifts(offsets_frames, pairs):
    o = np.asarray(offsets_frames, dtype=np.float64)
    return o[np.asarray(pairs)[:, 0]] - o[np.asarray(pairs)[:, 1]]


# ---- the recovery cases of tests/test_sync_ref.py and their bars (its docstring says where they come from) ------------------------------
# name: (V, N, planted offsets in frames, seed); each runs calibrated and uncalibrated, noise-free and with 2 px of noise
RECOVERY = {'three_views': (3, 90, (0.0, 3.3, -4.75), 700), 'four_views': (4, 150, (0.0, -2.25, 8.0, 5.7), 701)}
RECOVERY_OPTIONS = dict(max_offset_s=0.5)                                # +-15 frames at 30 fps; every other option is the tool's default
# (calibrated, noise px): (worst pair shift, worst offset) in frames: twice the worst measured over the two cases
# (profiles/sync_parity.json, group `recovery`)
RECOVERY_BARS = {(True, 0.0): (0.0018, 0.00072), (True, 2.0): (0.224, 0.165), (False, 0.0): (0.165, 0.126), (False, 2.0): (0.358, 0.214)}

# ---- the cases tests/test_gpu_sync.py runs, built once and shared ---------------------------------------------------------------------
# name: (V, N, J, Q, S, seed, non-finite E).  The seeds are held to the margins on the CPU (tests/test_sync_ref.py::
# test_margins_of_the_gpu_inputs): a seed that stops holding is replaced here with a comment, never skipped at run time.
SWEEP_CASES = {
    'one_pair': (2, 3, 22, 1, 7, 801, False),
    'one_pair_E_not_finite': (2, 3, 22, 1, 7, 801, True),
    'many_points': (4, 70, 25, 6, 33, 802, True),
    'sixteen_views': (16, 5, 22, 120, 3, 803, True),
}
_CASES = {}


def case_shifts(N, Q, S, seed):
    """[Q,S] shifts: integers, negative ones, fractions (none within 1e-3 of an integer), shifts beyond +-N and exactly one NaN per
    pair."""
    g = np.random.Generator(np.random.PCG64(seed))
    reach = min(N + 2, 9)
    sh = np.zeros((Q, S))
    for q in range(Q):
        row = []
        for k in range(S):
            kind = (k + q) % 3
            base = float(g.integers(-reach, reach + 1))
            row.append(base if kind == 0 else base + g.uniform(0.05, 0.95) if kind == 1 else -abs(base) - g.uniform(0.05, 0.95))
        row = np.array(row)
        row[0] = float(q % 2)                                              # an integer shift that leaves an overlap
        row[(q + 1) % S if S > 1 else 0] = np.nan
        sh[q] = row
    if S >= 7:
        sh[0, 3], sh[0, 4], sh[0, 5] = float(N), -float(N) - 0.5, float(N - 1)      # no overlap, none, the last frame alone
    return sh


def build_sweep_case(name):
    """-> {'keypoints', 'cams' (identity extrinsics), 'pairs', 'E', 'shifts', 'ref' [Q,S,4], 'margin_tau', 'margin_index'}; cached."""
    if name in _CASES:
        return _CASES[name]
    from rohm_amd import sync
    from rohm_amd.multiview import pack_cameras
    V, N, J, Q, S, seed, bad_E = SWEEP_CASES[name]
    g = np.random.Generator(np.random.PCG64(seed + 7))
    offsets = np.concatenate([[0.0], g.uniform(-2.0, 2.0, V - 1)])
    K, W, D, kp = make_scene(V, N, J, seed, offsets, noise_px=2.0)
    kp = MR.salt(kp, seed + 3000)
    if N >= 3:                                                             # salt() blinds frame 1; give it back to all but view 0
        kp[1:, 1, :, 2] = 0.9
    cams = pack_cameras(K, np.broadcast_to(np.eye(4), (V, 4, 4)), D)
    pairs = np.stack(np.triu_indices(V, 1), 1).astype(np.int32)
    assert len(pairs) == Q
    E = np.stack([sync.essential(W, a, b) for a, b in pairs])
    if Q >= 3:
        pairs = pairs.copy()
        pairs[1] = (pairs[1, 0], V)                                        # outside [0, V)
    if Q >= 6:
        pairs[2] = (2, 2)                                                  # v1 = v2
    if bad_E:
        E[Q - 1 if Q < 6 else 3, 4] = np.nan if Q != 6 else np.inf
    shifts = case_shifts(N, Q, S, seed + 11)
    ref, mt, mi = pair_sweep(kp, cams, pairs, E, shifts, with_margins=True)
    case = {'keypoints': kp, 'cams': cams, 'pairs': pairs, 'E': E, 'shifts': shifts, 'ref': ref, 'margin_tau': mt, 'margin_index': mi}
    for a in (kp, cams, pairs, E, shifts):
        a.setflags(write=False)
    _CASES[name] = case
    return case


def build_resample_case(name):
    """The keypoints of a sweep case with per-view shifts: zero, an integer, fractions, one beyond the recording, one NaN."""
    key = 'resample_' + name
    if key in _CASES:
        return _CASES[key]
    case = build_sweep_case(name)
    V, N = case['keypoints'].shape[:2]
    g = np.random.Generator(np.random.PCG64(SWEEP_CASES[name][5] + 13))
    shifts = g.uniform(-0.45 * N, 0.45 * N, V)
    shifts[0] = 0.0
    shifts[1] = 1.0 if N > 1 else 0.0
    if V > 2:
        shifts[2] = np.nan
    if V > 3:
        shifts[3] = N + 0.5
    if V > 4:
        shifts[4] = -2.0
    out = {'keypoints': case['keypoints'], 'shifts': shifts, 'ref': resample(case['keypoints'], shifts)}
    shifts.setflags(write=False)
    _CASES[key] = out
    return out


# the end-to-end case of tests/test_gpu_sync.py: V, N, J, planted offsets in frames, seed, the options of the tool
END_TO_END = dict(V=3, N=40, J=22, offsets=(0.0, 1.37, -2.6), seed=811, noise_px=0.5, max_offset_s=5.0 / FPS, hypotheses=64, rounds=6)
# twice the restatement's own offset error on that scene in frames (profiles/sync_parity.json, group `end_to_end_cpu`: 0.0118, 0.0101)
END_TO_END_BARS = {'calibrated': 0.024, 'uncalibrated': 0.021}
