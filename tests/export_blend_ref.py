"""TEST INFRASTRUCTURE ONLY: float64 numpy restatement of the blended export (csrc/export.hip `export_smplx_blend_kernel`,
include/rohm_hip.h rohm_export_smplx_blend) and of `rohm_amd.export.plan_blend`.

Built from the two restatements the project has already: tests/export_ref.py `export_params` makes the two candidates of a
frame, tests/track_ref.py `slerp_rotvec` / `geodesic` blend and compare them.  Nothing of the rule is restated twice."""
import numpy as np

import export_ref as ER
import track_ref as TR

ROT_COLS = TR.ROT_COLS


def plan_blend(starts, rows):
    """The plan rule, frame by frame (the package's `plan_blend` works on slices): -> (clip_a, t_a, clip_b, t_b, alpha, n)."""
    s = [int(v) for v in starts]
    hi = [v + rows for v in s]
    for c in range(1, len(s)):
        if s[c] > hi[c - 1]:
            raise ValueError(f'clips of {rows} rows at starts {s} leave frames uncovered')
    lo = [0 if c == 0 else s[c] if c == 1 else max(s[c], hi[c - 2]) for c in range(len(s))]
    n = hi[-1]
    out = []
    for f in range(n):
        active = [c for c in range(len(s)) if lo[c] <= f < hi[c]]
        assert 1 <= len(active) <= 2, (f, active)
        if len(active) == 1:
            out.append((active[0], f - s[active[0]], -1, 0, 0.0))
        else:
            a, b = active
            assert b == a + 1
            m, i = hi[a] - lo[b], f - lo[b]
            out.append((a, f - s[a], b, f - s[b], (i + 1) / (m + 1)))
    cols = list(zip(*out))
    return (np.array(cols[0], np.int32), np.array(cols[1], np.int32), np.array(cols[2], np.int32), np.array(cols[3], np.int32),
            np.array(cols[4], np.float64), n)


def pelvis_position(params, pelvis):
    """transl + d(betas) [N, 3]: where SMPL-X puts the pelvis of rows [N, 79] (pelvis = export_ref.fold_pelvis(...))."""
    Jt, Js = (np.asarray(v, np.float32).astype(np.float64) for v in pelvis)
    return params[:, 3:6] + Jt + params[:, 6:16] @ Js.T


def blend_rows(pa, ca, pb, cb, two, alpha, pelvis):
    """Candidates a / b as rows [N, 79] float64 with contact [N, 4] float32, `two` [N] bool (b exists), alpha [N] ->
    (params, contact, disagree [N, 23]).  One candidate or alpha == 0: candidate a's rows."""
    alpha = np.asarray(alpha, np.float64)
    fade = two & (alpha != 0.0)
    out, contact, dis = pa.copy(), ca.copy(), np.zeros((len(pa), 23))
    al = alpha[fade]
    out[fade, 3:16] = pa[fade, 3:16] + al[:, None] * (pb[fade, 3:16] - pa[fade, 3:16])
    for j, c in enumerate(ROT_COLS):
        out[fade, c:c + 3] = TR.slerp_rotvec(pa[fade, c:c + 3], pb[fade, c:c + 3], al)
        dis[two, j] = TR.geodesic(pa[two, c:c + 3], pb[two, c:c + 3])
    a64, b64 = ca[fade].astype(np.float64), cb[fade].astype(np.float64)
    contact[fade] = (a64 + al[:, None] * (b64 - a64)).astype(np.float32)
    d = pelvis_position(pb[two], pelvis) - pelvis_position(pa[two], pelvis)
    dis[two, 22] = np.sqrt((d * d).sum(-1))
    return out, contact, dis


def export_blend(repr_clips, plan, pelvis, transf=None, rigid=None, mean=None, std=None):
    """repr_clips [C, T, 294] float32, plan = (clip_a, t_a, clip_b, t_b, alpha) -> (params [N, 79] float64, contact [N, 4]
    float32, disagree [N, 23] float64).  An index outside [0, C) x [0, T) on the a side, or on the b side where clip_b >= 0,
    gives a NaN row in all three."""
    fa, ta, fb, tb, alpha = (np.asarray(v) for v in plan[:5])
    two = fb >= 0
    kw = dict(transf=transf, rigid=rigid, mean=mean, std=std)
    pa, ca = ER.export_params(repr_clips, fa, ta, pelvis, **kw)
    pb, cb = ER.export_params(repr_clips, np.where(two, fb, fa), np.where(two, tb, ta), pelvis, **kw)
    bad = np.isnan(pa).any(axis=1) | np.isnan(pb).any(axis=1)
    ok = ~bad
    params, contact, dis = np.full((len(fa), 79), np.nan), np.full((len(fa), 4), np.nan, np.float32), np.full((len(fa), 23), np.nan)
    params[ok], contact[ok], dis[ok] = blend_rows(pa[ok], ca[ok], pb[ok], cb[ok], two[ok], np.asarray(alpha, np.float64)[ok], pelvis)
    return params, contact, dis


def rotation_error(got, want):
    """Largest geodesic angle (rad) between the 22 rotations of two sets of rows [N, 79]."""
    if len(got) == 0:
        return 0.0
    return float(max(TR.geodesic(got[:, c:c + 3], want[:, c:c + 3]).max() for c in ROT_COLS))


# ---- shared synthetic clips ------------------------------------------------------------------------------------------------
def _rot6d(R, g):
    """Rotation matrices [..., 3, 3] -> interleaved 6-D vectors that are neither unit nor orthogonal (Gram-Schmidt has work)."""
    a1 = R[..., :, 0] * g.uniform(0.7, 1.4, size=R.shape[:-2] + (1,))
    a2 = R[..., :, 1] * g.uniform(0.7, 1.4, size=R.shape[:-2] + (1,)) + g.uniform(-0.2, 0.2, size=R.shape[:-2] + (1,)) * R[..., :, 0]
    return np.stack([a1, a2], axis=-1).reshape(R.shape[:-2] + (6,))


def overlapping_clips(starts, rows, seed):
    """Clips [C, rows, 294] float32 (de-normalised) at `starts` that tell nearly the same story about every scene frame they
    share, and their scene -> canonical transforms [C, 4, 4] float32: a smooth scene track (track_ref.smooth_params), per
    clip a yaw of at most 0.4 rad and a shift, per row a perturbation of at most 0.3 rad per rotation, 3 cm, 0.05 in betas.
    Two candidates of a frame are therefore less than 2 rad apart in every setting of transf / rigid (0.8 + 0.6 < 2)."""
    g = np.random.Generator(np.random.PCG64(seed))
    n = int(starts[-1]) + rows
    scene = TR.smooth_params(g, n, step_angle=0.08)
    C = len(starts)
    rep = g.standard_normal((C, rows, 294)).astype(np.float32)
    transf = np.zeros((C, 4, 4), np.float32)
    for c, s in enumerate(starts):
        yaw = np.array([0.0, 0.0, g.uniform(-0.4, 0.4)])
        Rc = ER.rodrigues(yaw)
        tc = g.uniform(-0.5, 0.5, size=3)
        transf[c, :3, :3], transf[c, :3, 3], transf[c, 3, 3] = Rc, tc, 1.0
        rows_scene = scene[s:s + rows]
        rv = np.stack([rows_scene[:, k:k + 3] for k in ROT_COLS], axis=1)                      # [rows, 22, 3]
        rv = TR.compose(rv, TR.random_rotvecs(g, (rows, 22), 0.3))
        R = ER.rodrigues(rv)
        R[:, 0] = Rc @ R[:, 0]
        six = _rot6d(R, g)
        rep[c, :, ER.CH_ROT6D:ER.CH_ROT6D + 6] = six[:, 0]
        rep[c, :, ER.CH_POSE6D:ER.CH_POSE6D + 126] = six[:, 1:].reshape(rows, 126)
        rep[c, :, ER.CH_TRANS:ER.CH_TRANS + 3] = rows_scene[:, 3:6] @ Rc.T + tc + g.uniform(-0.03, 0.03, size=(rows, 3))
        rep[c, :, ER.CH_BETAS:ER.CH_BETAS + 10] = rows_scene[:, 6:16] + g.uniform(-0.05, 0.05, size=(rows, 10))
        rep[c, :, ER.CH_CONTACT:ER.CH_CONTACT + 4] = g.uniform(0.0, 1.0, size=(rows, 4))
    return rep, transf


LAYOUTS = {'regular': [0, 10, 20], 'heavy': [0, 5, 10, 15], 'tail': [0, 10, 20, 23]}
ROWS = 16
