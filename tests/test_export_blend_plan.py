"""Host: the cross-fade plan of the export (`rohm_amd.export.plan_blend`) over regular windows, heavy overlaps and the track
loader's tail clip, the restatement of the blended export (tests/export_blend_ref.py) against itself and against scipy, and
the command line's `--keep blend`."""
import numpy as np
import pytest

import export_blend_ref as BR
import export_ref as ER
import track_ref as TR

ROWS = BR.ROWS
LAYOUTS = dict(BR.LAYOUTS, heavy=list(range(0, 45, 5)))          # stride 5 for nine clips: every clip after the second is trimmed


def _active(starts, rows):
    hi = [s + rows for s in starts]
    lo = [0 if c == 0 else starts[c] if c == 1 else max(starts[c], hi[c - 2]) for c in range(len(starts))]
    return lo, hi


@pytest.mark.parametrize('name', sorted(LAYOUTS))
def test_plan_covers_every_frame_with_at_most_two_clips(name):
    from rohm_amd.export import plan_blend
    starts = LAYOUTS[name]
    ca, ta, cb, tb, alpha, n = plan_blend(starts, ROWS)
    assert n == starts[-1] + ROWS and all(len(v) == n for v in (ca, ta, cb, tb, alpha))
    assert ca.dtype == ta.dtype == cb.dtype == tb.dtype == np.int32 and alpha.dtype == np.float64
    want = BR.plan_blend(starts, ROWS)                                # the rule frame by frame (asserts <= 2 active clips per frame)
    for got, ref in zip((ca, ta, cb, tb, alpha), want):
        assert np.array_equal(got, ref)
    lo, hi = _active(starts, ROWS)
    f = np.arange(n)
    count = sum(((f >= lo[c]) & (f < hi[c])).astype(int) for c in range(len(starts)))
    assert count.min() >= 1 and count.max() <= 2                      # covered; never a third clip
    shared = count == 2
    assert np.array_equal(shared, cb >= 0) and np.array_equal(shared, (alpha > 0) & (alpha < 1))
    assert (cb[~shared] == -1).all() and (tb[~shared] == 0).all() and (alpha[~shared] == 0).all()
    assert (ta >= 0).all() and (ta < ROWS).all() and (tb >= 0).all() and (tb < ROWS).all()
    s = np.asarray(starts)
    assert np.array_equal(s[ca] + ta, f) and np.array_equal((s[np.maximum(cb, 0)] + tb)[shared], f[shared])      # rows are f - starts[clip]
    assert (cb[shared] == ca[shared] + 1).all()
    for c in range(1, len(starts)):                                   # every seam: the closed form, strictly increasing
        m = hi[c - 1] - lo[c]
        seam = alpha[lo[c]:hi[c - 1]]
        assert np.array_equal(seam, (np.arange(m) + 1.0) / (m + 1.0)) and (np.diff(seam) > 0).all()
        assert (ca[lo[c]:hi[c - 1]] == c - 1).all() and (cb[lo[c]:hi[c - 1]] == c).all()
    if name == 'heavy':
        assert any(lo[c] > starts[c] for c in range(2, len(starts)))          # trimming did occur
    if name == 'tail':
        assert starts[3] < hi[1] and lo[3] == hi[1] == 26                      # the tail clip overlapped two predecessors


def test_plan_edge_cases():
    from rohm_amd.export import plan_blend
    ca, ta, cb, tb, alpha, n = plan_blend([0, 16, 32], 16)            # abutting clips (m = 0) blend nothing
    assert n == 48 and (cb == -1).all() and (alpha == 0).all() and ca.tolist() == [0] * 16 + [1] * 16 + [2] * 16
    ca, ta, cb, tb, alpha, n = plan_blend([0], 7)
    assert n == 7 and ca.tolist() == [0] * 7 and ta.tolist() == list(range(7)) and (cb == -1).all()
    assert plan_blend([], 16)[5] == 0 and len(plan_blend([], 16)[4]) == 0
    with pytest.raises(ValueError, match='leave frames uncovered'):
        plan_blend([0, 17], 16)
    with pytest.raises(ValueError, match='leave frames uncovered'):
        plan_blend([0, 10, 27], 16)
    with pytest.raises(ValueError):
        plan_blend([1, 10], 16)
    with pytest.raises(ValueError):
        plan_blend([0, 10, 10], 16)
    # regular windows are arange(C) * (clip_len - overlap_len)
    ca, _, cb, _, alpha, n = plan_blend(np.arange(3) * (17 - 6), 16)
    assert n == 38 and (cb >= 0).sum() == 10 and np.allclose(alpha[11:16], np.arange(1, 6) / 6.0, rtol=0, atol=0)


# ---- the restatement against itself ------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def candidates():
    g = np.random.Generator(np.random.PCG64(11))
    n = 40
    pa = TR.smooth_params(g, n)
    pb = pa.copy()
    for c in TR.ROT_COLS:
        pb[:, c:c + 3] = TR.compose(pa[:, c:c + 3], TR.random_rotvecs(g, (n,), 1.9))          # < 2 rad apart
    pb[:, 3:16] += g.uniform(-0.1, 0.1, size=(n, 13))
    ca, cb = g.uniform(size=(n, 4)).astype(np.float32), g.uniform(size=(n, 4)).astype(np.float32)
    pelvis = (g.standard_normal(3).astype(np.float32) * 0.1, g.standard_normal((3, 10)).astype(np.float32) * 0.01)
    return pa, ca, pb, cb, g.uniform(0.02, 0.98, size=n), pelvis


def test_restatement_alpha_zero_is_candidate_a(candidates):
    pa, ca, pb, cb, alpha, pelvis = candidates
    two = np.ones(len(pa), bool)
    out, contact, dis = BR.blend_rows(pa, ca, pb, cb, two, np.zeros(len(pa)), pelvis)
    assert np.array_equal(out, pa) and np.array_equal(contact, ca) and (dis[:, :22] > 0).all()
    out, contact, dis = BR.blend_rows(pa, ca, pb, cb, ~two, alpha, pelvis)
    assert np.array_equal(out, pa) and np.array_equal(contact, ca) and not dis.any()
    out, _, _ = BR.blend_rows(pa, ca, pb, cb, two, np.full(len(pa), 1e-13), pelvis)          # alpha -> 0 arrives at a
    assert BR.rotation_error(out, pa) <= 1e-12 and np.abs(out[:, 3:16] - pa[:, 3:16]).max() <= 1e-12


def test_restatement_is_symmetric(candidates):
    pa, ca, pb, cb, alpha, pelvis = candidates
    two = np.ones(len(pa), bool)
    ab, c_ab, d_ab = BR.blend_rows(pa, ca, pb, cb, two, alpha, pelvis)
    ba, c_ba, d_ba = BR.blend_rows(pb, cb, pa, ca, two, 1.0 - alpha, pelvis)
    assert BR.rotation_error(ab, ba) <= 1e-12 and np.abs(ab[:, 3:16] - ba[:, 3:16]).max() <= 1e-12
    assert np.abs(d_ab - d_ba).max() <= 1e-12 and np.abs(c_ab.astype(np.float64) - c_ba).max() <= 1e-6
    assert 0.0 < d_ab[:, :22].max() < 2.0
    assert np.abs(d_ab[:, 22] - np.linalg.norm(BR.pelvis_position(pa, pelvis) - BR.pelvis_position(pb, pelvis), axis=1)).max() <= 1e-15


def test_restatement_slerp_is_scipy(candidates):
    from scipy.spatial.transform import Rotation, Slerp
    pa, ca, pb, cb, alpha, pelvis = candidates
    out, _, dis = BR.blend_rows(pa, ca, pb, cb, np.ones(len(pa), bool), alpha, pelvis)
    worst = worst_dis = 0.0
    for n in range(len(pa)):
        for j, c in enumerate(TR.ROT_COLS):
            key = Rotation.from_rotvec(np.stack([pa[n, c:c + 3], pb[n, c:c + 3]]))
            want = Slerp([0.0, 1.0], key)([alpha[n]]).as_rotvec()[0]
            worst = max(worst, float(TR.geodesic(out[n, c:c + 3], want)))
            worst_dis = max(worst_dis, abs(dis[n, j] - (key[0].inv() * key[1]).magnitude()))
    print(f'restatement slerp against scipy: {worst:.3e} rad; disagreement against scipy: {worst_dis:.3e} rad')
    assert worst <= 1e-12 and worst_dis <= 1e-12


def test_restatement_on_synthetic_clips_keeps_candidates_close():
    """The clips the GPU tests use: two candidates of a frame stay less than 2 rad apart, where no shortest arc is ambiguous."""
    for name, starts in BR.LAYOUTS.items():
        rep, transf = BR.overlapping_clips(starts, ROWS, seed=3)
        plan = BR.plan_blend(starts, ROWS)
        pelvis = (np.zeros(3, np.float32), np.zeros((3, 10), np.float32))
        for tf in (None, transf):
            params, contact, dis = BR.export_blend(rep, plan, pelvis, transf=tf)
            assert np.isfinite(params).all() and 0.0 < dis[:, :22].max() < 2.0, (name, dis[:, :22].max())
            single = plan[2] < 0
            first, first_contact = ER.export_params(rep, plan[0], plan[1], pelvis, transf=tf)
            assert np.array_equal(params[single], first[single]) and np.array_equal(contact[single], first_contact[single])
            assert not dis[single].any() and (dis[~single, :22] > 0).all()


# ---- the interface --------------------------------------------------------------------------------------------------------
def test_command_line_accepts_keep_blend():
    from rohm_amd.export import parse_args
    args = parse_args(['--keep', 'blend', '--dataset', 'track', '--saved_data_path', 'walk.pkl'])
    assert args.keep == 'blend'
    assert parse_args(['--saved_data_path', 'walk.pkl']).keep == 'first'
    with pytest.raises(SystemExit):
        parse_args(['--keep', 'both', '--saved_data_path', 'walk.pkl'])


def test_export_plan_of_the_track_loader_blends():
    from rohm_amd.data_loaders.track import DataloaderTrack
    from rohm_amd.export import plan_blend
    ds = DataloaderTrack.__new__(DataloaderTrack)                     # the method only reads clip_starts and clip_len
    ds.clip_starts, ds.clip_len = np.array([0, 10, 20, 23], np.int32), 17
    got = ds.export_plan(keep='blend', rows=16)
    for a, b in zip(got, plan_blend([0, 10, 20, 23], 16)):
        assert np.array_equal(a, b)
    assert ds.export_plan(keep='blend')[5] == 40 and len(ds.export_plan('first')) == 3
