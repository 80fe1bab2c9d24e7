"""GPU: the blended export -- `rohm_export_smplx_blend` (csrc/export.hip) against its float64 restatement
(tests/export_blend_ref.py, built from export_ref.py and track_ref.py), bit for bit against `rohm_export_smplx` wherever one
clip gives the frame, on identical evidence, on a seam with a closed form, on bad indices and stale output buffers, and
through the track driver and the command line.

Kernel and restatement are both float64 on the same float32 inputs and differ by libm and fma contraction only; the bars are
tests/test_gpu_export.py's KERNEL_BAR = 1e-9: absolute on transl / betas, 1e-9 rad geodesic on the 22 rotations (by geodesic,
not by component: at pi the sign of a rotation vector is arbitrary), 1e-9 on `disagree`, 1e-6 on the float32 contact.  Two
candidates of a frame are less than 2 rad apart everywhere, so no shortest arc is ambiguous.  The measured maxima go to
profiles/export_blend_parity.json."""
import json
import math
import os

import numpy as np
import pytest
import torch

import export_blend_ref as BR
import export_ref as ER
import stale_memory as SM
import track_ref as TR
from helpers import golden
from rohm_amd.utils import synth
from test_gpu_track import _common, _load, body_dir, holed_25fps_track, scene  # noqa: F401  (body_dir, scene: fixtures)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_BAR = 1e-9                      # tests/test_gpu_export.py
CONTACT_BAR = 1e-6
ROWS = BR.ROWS
PARITY = {}


def _record(key, value):
    path = os.path.join(ROOT, 'profiles', 'export_blend_parity.json')
    PARITY[key] = max(float(value), PARITY.get(key, 0.0))
    try:
        with open(path) as f:
            data = json.load(f)
    except (OSError, ValueError):
        data = {}
    data.setdefault('gpu', {}).update(PARITY)
    try:
        with open(path, 'w') as f:
            json.dump(data, f, indent=1, sort_keys=True)
            f.write('\n')
    except OSError:
        pass


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _layer(tensors):
    from rohm_amd.body_model import SMPLXLayer
    return SMPLXLayer.from_tensors(tensors).to(DEV)


@pytest.fixture(scope='module')
def small():
    """The 419-vertex synthetic body model of tests/test_gpu_export.py, statistics and a camera."""
    from rohm_amd.body_model import native_for
    tensors = synth.synthetic_smplx_tensors(0, num_verts=int(golden('export.npz')['num_verts']))
    layer = _layer(tensors)
    mean, std = synth.synthetic_stats(3)
    cam2world = np.eye(4)
    cam2world[:3, :3] = ER.rodrigues(np.array([0.25, -0.5, 0.15]))
    cam2world[:3, 3] = [0.4, -1.1, 2.2]
    return {'tensors': tensors, 'layer': layer, 'handle': native_for(layer, torch.device(DEV)).handle, 'pelvis': ER.fold_pelvis(tensors),
            'mean': mean.astype(np.float32), 'std': std.astype(np.float32), 'rigid': np.linalg.inv(cam2world), 'cam2world': cam2world}


_CLIPS, _WANT = {}, {}


def _clips(small, name):
    """Overlapping clips [C, 16, 294] of one layout (de-normalised and normalised), their transforms and the blend plan."""
    if name not in _CLIPS:
        from rohm_amd.export import plan_blend
        starts = BR.LAYOUTS[name]
        rep, transf = BR.overlapping_clips(starts, ROWS, seed=3)
        _CLIPS[name] = {'rep': rep, 'rep_norm': ((rep - small['mean']) / small['std']).astype(np.float32), 'transf': transf,
                        'plan': plan_blend(starts, ROWS)}
    return _CLIPS[name]


def _launch(small, rep, transf_arr, layout, plan, stats, transf, rigid, **kw):
    from rohm_amd import ops
    x = _dev(rep)
    if layout == 'bc1t':
        x = x.permute(0, 2, 1).unsqueeze(2).contiguous()          # [C, 294, 1, T]
    idx = [_dev(np.asarray(v), torch.int32) for v in plan[:4]]
    return ops.export_smplx_blend(small['handle'], x, layout, *idx, _dev(np.asarray(plan[4], np.float64)),
                                  transf=_dev(transf_arr) if transf else None, rigid=_dev(small['rigid']) if rigid else None,
                                  mean=_dev(small['mean']) if stats else None, std=_dev(small['std']) if stats else None, **kw)


def _launch_plain(small, rep, transf_arr, layout, fc, ft, stats, transf, rigid):
    from rohm_amd import ops
    x = _dev(rep)
    if layout == 'bc1t':
        x = x.permute(0, 2, 1).unsqueeze(2).contiguous()
    return ops.export_smplx(small['handle'], x, layout, _dev(np.asarray(fc), torch.int32), _dev(np.asarray(ft), torch.int32),
                            transf=_dev(transf_arr) if transf else None, rigid=_dev(small['rigid']) if rigid else None,
                            mean=_dev(small['mean']) if stats else None, std=_dev(small['std']) if stats else None)


def _restate(small, name, stats, transf, rigid):
    key = (name, stats, transf, rigid)
    if key not in _WANT:
        c = _clips(small, name)
        _WANT[key] = BR.export_blend(c['rep_norm'] if stats else c['rep'], c['plan'], small['pelvis'], transf=c['transf'] if transf else None,
                                     rigid=small['rigid'] if rigid else None, mean=small['mean'] if stats else None,
                                     std=small['std'] if stats else None)
    return _WANT[key]


# ---- kernel against restatement --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rigid', [False, True])
@pytest.mark.parametrize('transf', [False, True])
@pytest.mark.parametrize('stats', [False, True])
@pytest.mark.parametrize('layout', ['btc', 'bc1t'])
@pytest.mark.parametrize('name', ['regular', 'heavy', 'tail'])
def test_kernel_matches_the_restatement(small, name, layout, stats, transf, rigid):
    c = _clips(small, name)
    N = c['plan'][5]
    assert N == {'regular': 36, 'heavy': 31, 'tail': 39}[name] and N % 8 and N <= 64          # a workgroup with idle frame slots
    params, contact, disagree = _launch(small, c['rep_norm'] if stats else c['rep'], c['transf'], layout, c['plan'], stats, transf, rigid)
    assert tuple(params.shape) == (N, 79) and params.dtype == torch.float64
    assert tuple(contact.shape) == (N, 4) and contact.dtype == torch.float32
    assert tuple(disagree.shape) == (N, 23) and disagree.dtype == torch.float64
    want, want_contact, want_dis = _restate(small, name, stats, transf, rigid)
    shared = c['plan'][2] >= 0
    assert 0.0 < want_dis[shared, :22].max() < 2.0 and (want_dis[shared, :22] > 0).all()      # every case counts: none is ambiguous
    got = params.cpu().numpy()
    assert np.isfinite(got).all()
    rot = BR.rotation_error(got, want)
    lin = np.abs(got[:, 3:16] - want[:, 3:16]).max()
    dis = np.abs(disagree.cpu().numpy() - want_dis).max()
    con = np.abs(contact.cpu().numpy().astype(np.float64) - want_contact).max()
    print(f'{name} {layout} stats={stats} transf={transf} rigid={rigid}: rotations {rot:.3e} rad, transl / betas {lin:.3e}, '
          f'disagree {dis:.3e}, contact {con:.3e}')
    _record('kernel_vs_restatement_rotation_max_geodesic_rad', rot)
    _record('kernel_vs_restatement_transl_betas_max_abs', lin)
    _record('kernel_vs_restatement_disagree_max_abs', dis)
    _record('kernel_vs_restatement_contact_max_abs', con)
    assert rot <= KERNEL_BAR and lin <= KERNEL_BAR and dis <= KERNEL_BAR and con <= CONTACT_BAR
    assert max(np.linalg.norm(got[:, k:k + 3], axis=-1).max() for k in TR.ROT_COLS) <= math.pi + 1e-12
    assert not disagree[_dev(~shared)].any()
    again = _launch(small, c['rep_norm'] if stats else c['rep'], c['transf'], layout, c['plan'], stats, transf, rigid)
    assert all(torch.equal(a, b) for a, b in zip(again, (params, contact, disagree)))         # no atomics: the same bits


# ---- bitwise against the existing export -------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout', ['btc', 'bc1t'])
@pytest.mark.parametrize('name', ['regular', 'heavy', 'tail'])
def test_single_clip_frames_are_the_plain_export_bit_for_bit(small, name, layout):
    from rohm_amd.data_loaders.track import frames_plan
    c = _clips(small, name)
    fc, ft, n = frames_plan(BR.LAYOUTS[name], ROWS, 'first')
    assert n == c['plan'][5]
    params, contact, disagree = _launch(small, c['rep_norm'], c['transf'], layout, c['plan'], True, True, True)
    first, first_contact = _launch_plain(small, c['rep_norm'], c['transf'], layout, fc, ft, True, True, True)
    single = _dev(c['plan'][2] < 0)
    assert 0 < int(single.sum()) < n
    assert torch.equal(params[single], first[single]) and torch.equal(contact[single], first_contact[single])
    assert not torch.equal(params[~single], first[~single])
    # nothing to blend anywhere (all clip_b = -1), for 'first' and for 'last': the plain export over the whole track
    for keep in ('first', 'last'):
        fc, ft, n = frames_plan(BR.LAYOUTS[name], ROWS, keep)
        plan = (fc, ft, np.full(n, -1, np.int32), np.zeros(n, np.int32), np.zeros(n))
        params, contact, disagree = _launch(small, c['rep_norm'], c['transf'], layout, plan, True, True, True)
        plain, plain_contact = _launch_plain(small, c['rep_norm'], c['transf'], layout, fc, ft, True, True, True)
        assert torch.equal(params, plain) and torch.equal(contact, plain_contact) and not disagree.any()
    # ... and alpha == 0 with a second candidate: candidate a's bits, the disagreement still reported
    plan = c['plan'][:4] + (np.zeros(n),)
    params, contact, disagree = _launch(small, c['rep_norm'], c['transf'], layout, plan, True, True, True)
    plain, plain_contact = _launch_plain(small, c['rep_norm'], c['transf'], layout, plan[0], plan[1], True, True, True)
    assert torch.equal(params, plain) and torch.equal(contact, plain_contact) and (disagree[~single, :22] > 0).all()


# ---- identical evidence --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def big():
    tensors = synth.synthetic_smplx_tensors(0)
    return tensors, _layer(tensors)


def _scene_motion(n, period=None, seed=5):
    """Camera-frame parameters of a body that sways about an upright pose (scripts/bench_track.py's motion).  With `period` the
    motion repeats every `period` frames bit for bit: one period is computed and tiled."""
    g = np.random.Generator(np.random.PCG64(seed))
    m = n if period is None else period
    k = g.integers(1, 3, size=79) if period is not None else g.uniform(0.3, 1.2, size=79) * m / 30.0
    p = 0.35 * np.sin(2 * np.pi * k * np.arange(m)[:, None] / m + g.uniform(0, 2 * np.pi, size=79))
    p[:, 3:6] = 0.1 * p[:, 3:6] + np.array([0.0, 0.0, 3.0])
    p[:, 6:16] = g.standard_normal(10) * 0.3
    p[:, 0:3] += np.array([np.pi / 2, 0.0, 0.0]) * 0.9
    if period is not None:
        p = np.tile(p, (-(-n // period), 1))[:n]
    cam2world = np.eye(4)
    cam2world[:3, :3] = np.array([[1.0, 0, 0], [0, 0, 1.0], [0, -1.0, 0]])
    return {key: p[:, a:b].astype(np.float32) for key, (a, b) in ER.PARAM_COLS.items()}, cam2world


@pytest.mark.parametrize('motion', ['periodic', 'free'])
def test_identical_evidence_is_left_alone(big, motion):
    """Clips cut by `clips.build_clips` (clip_len 17, overlap_len 6: three clips, stride 11, 5 shared frames per seam) from one
    continuous scene motion.  The representation is float32 in every clip's own canonical frame, so two clips say the same
    about a shared frame only to float32 rounding.  'periodic' makes their evidence identical: the motion repeats every 11
    frames bit for bit, every clip is cut from the same bits and a shared frame is the same scene pose in both -- there the
    blend must be the plain export within 1e-9.  'free' is a motion without a period: the candidates differ by the float32
    representation, `disagree` stays below the loader round trip's bar and so does the blend's distance from 'first'."""
    from rohm_amd.data_loaders import clips, frames
    from rohm_amd.export import export_params, plan_frames
    L, OVERLAP = 17, 6
    stride = L - OVERLAP
    n = 2 * stride + L
    prm, cam2world = _scene_motion(n, period=stride if motion == 'periodic' else None)
    mean, std = synth.synthetic_stats(3)
    joints_world, smplx_world = frames.frames_to_world(big[1], prm, cam2world, DEV)
    built = clips.build_clips(joints_world, smplx_world, L, OVERLAP, up_axis='z', preset_floor_height=-0.05, stats=(mean, std))
    assert tuple(built['repr'].shape) == (3, L - 1, 294)
    kw = dict(clip_len=L, overlap_len=OVERLAP, stats=(mean, std), frame='scene')
    first = export_params(built['repr'], built['transf_matrix'], big[1], keep='first', **kw)
    blend = export_params(built['repr'], built['transf_matrix'], big[1], keep='blend', **kw)
    assert len(first) == len(blend) == n - 1 and first.disagree is None and int((blend.frame_clip_b >= 0).sum()) == 10
    a, b = blend.params79.cpu().numpy(), first.params79.cpu().numpy()
    rot, lin = BR.rotation_error(a, b), float(np.abs(a[:, 3:16] - b[:, 3:16]).max())
    dis = float(blend.disagree.max())
    bar = 4 * ER.roundtrip_cpu(golden('video_loader.npz'), big[0], plan_frames)['roundtrip_cpu_error']      # tests/test_gpu_export.py
    print(f'{motion}: blend against first: rotations {rot:.3e} rad, transl / betas {lin:.3e}; disagree {dis:.3e} (round-trip bar {bar:.3e})')
    _record(f'identical_evidence_{motion}_blend_vs_first_rotation_rad', rot)
    _record(f'identical_evidence_{motion}_blend_vs_first_transl_betas', lin)
    _record(f'identical_evidence_{motion}_disagree_max', dis)
    assert dis <= bar
    if motion == 'periodic':
        assert torch.equal(built['repr'][0], built['repr'][1]) and torch.equal(built['transf_matrix'][0], built['transf_matrix'][2])
        assert rot <= KERNEL_BAR and lin <= KERNEL_BAR
    else:
        assert rot <= bar and lin <= bar
    assert tuple(blend.joints.shape) == (n - 1, 22, 3) and torch.isfinite(blend.joints).all()


# ---- the seam, closed form ---------------------------------------------------------------------------------------------------
def _seam_transforms(small, rep):
    """Two scene -> canonical transforms that differ by a yaw of 0.2 rad about the pelvis and a shift of 0.1 m along the yaw
    axis.  A float32 matrix holds a generic yaw only to about 1e-8 rad and a generic shift to about 4e-9 m, which would drown
    the 1e-9 of this test: take the first yaw phi = 0.01 i and the first height z = -0.001 i whose float32 pair realises 0.2
    and 0.1 to 1e-10, measured in float64 with the restatement's functions."""
    R0 = ER.rot6d_to_rotmat(rep[0, 0, ER.CH_ROT6D:ER.CH_ROT6D + 6].astype(np.float64))

    def pair(phi, z):
        tf = np.zeros((2, 4, 4), np.float32)
        for c, (ang, h) in enumerate(((phi, z), (phi + 0.2, z + 0.1))):
            tf[c, :3, :3], tf[c, 2, 3], tf[c, 3, 3] = ER.rodrigues(np.array([0.0, 0.0, ang])), h, 1.0
        return tf

    def measured(tf):                                                 # the pelvis is the canonical origin: it lands on A's translation
        A = [ER.affine(t) for t in tf]
        ra, rb = (ER.rotmat_to_rotvec(a[:3, :3] @ R0) for a in A)
        return float(TR.geodesic(ra, rb)), float(np.linalg.norm(A[1][:3, 3] - A[0][:3, 3]))
    phi = next(0.01 * i for i in range(400) if abs(measured(pair(0.01 * i, 0.0))[0] - 0.2) <= 1e-10)
    z = next(-0.001 * i for i in range(400) if abs(measured(pair(phi, -0.001 * i))[1] - 0.1) <= 1e-10)
    tf = pair(phi, z)
    one = (np.zeros(1, np.int32), np.zeros(1, np.int32), np.ones(1, np.int32), np.zeros(1, np.int32), np.full(1, 0.5))
    dis = BR.export_blend(rep[:, :1], one, small['pelvis'], transf=tf)[2]          # ... and so says the whole restatement
    assert abs(dis[0, :22].max() - 0.2) <= 2e-10 and abs(dis[0, 22] - 0.1) <= 2e-10
    return tf


def test_seam_closed_form(small):
    from rohm_amd.export import export_params
    g = np.random.Generator(np.random.PCG64(8))
    m = 6
    L, OVERLAP = ROWS + 1, ROWS + 1 - (ROWS - m)                      # stride ROWS - m: the two clips share m frames
    row = g.standard_normal(294).astype(np.float32)
    R = ER.rodrigues(TR.random_rotvecs(g, (22,), 1.0))
    six = np.stack([R[:, :, 0], R[:, :, 1]], axis=-1).reshape(22, 6)
    row[ER.CH_ROT6D:ER.CH_ROT6D + 6], row[ER.CH_POSE6D:ER.CH_POSE6D + 126] = six[0], six[1:].reshape(126)
    row[ER.CH_BETAS:ER.CH_BETAS + 10] = 0.0
    row[ER.CH_TRANS:ER.CH_TRANS + 3] = -small['pelvis'][0]            # transl + d(betas) = 0: the yaw turns about the pelvis
    rep = np.broadcast_to(row, (2, ROWS, 294)).copy()                 # the same static canonical rows in both clips
    transf = _seam_transforms(small, rep)
    kw = dict(clip_len=L, overlap_len=OVERLAP, frame='scene')
    first = export_params(rep, transf, small['layer'], keep='first', **kw)
    blend = export_params(rep, transf, small['layer'], keep='blend', **kw)
    N = 2 * ROWS - m
    assert len(first) == len(blend) == N and int((blend.frame_clip_b >= 0).sum()) == m
    pel = lambda r: BR.pelvis_position(r.params79.cpu().numpy(), small['pelvis'])          # noqa: E731
    step = lambda p: np.linalg.norm(np.diff(p, axis=0), axis=1)                              # noqa: E731
    yaw = lambda r: TR.geodesic(r.params79.cpu().numpy()[:-1, 0:3], r.params79.cpu().numpy()[1:, 0:3])      # noqa: E731
    jump, jump_yaw = step(pel(first)).max(), yaw(first).max()
    assert jump >= 0.09 and jump_yaw >= 0.19                          # the pop of the plain export
    steps, yaws = step(pel(blend)), yaw(blend)
    dis = blend.disagree.cpu().numpy()
    shared = (blend.frame_clip_b >= 0).cpu().numpy()
    seam_angle, seam_dist = dis[:, :22].max(axis=1), dis[:, 22]
    print(f"'first': pelvis step {jump:.6f} m, yaw step {jump_yaw:.6f} rad; 'blend' over {m} frames: largest pelvis step {steps.max():.9f} m "
          f'(closed form {0.1 / (m + 1):.9f}), largest yaw step {yaws.max():.9f} rad ({0.2 / (m + 1):.9f}); seam_dist - 0.1 = '
          f'{np.abs(seam_dist[shared] - 0.1).max():.3e}, seam_angle - 0.2 = {np.abs(seam_angle[shared] - 0.2).max():.3e}')
    _record('seam_closed_form_pelvis_step_excess', steps.max() - 0.1 / (m + 1))
    _record('seam_closed_form_seam_dist_error', np.abs(seam_dist[shared] - 0.1).max())
    _record('seam_closed_form_seam_angle_error', np.abs(seam_angle[shared] - 0.2).max())
    assert (steps <= 0.1 / (m + 1) + 1e-9).all() and (yaws <= 0.2 / (m + 1) + 1e-9).all()
    assert np.abs(seam_dist[shared] - 0.1).max() <= 1e-9 and np.abs(seam_angle[shared] - 0.2).max() <= 1e-9
    assert not dis[~shared].any()
    assert int((steps > 0.1 / (m + 1) - 1e-9).sum()) == m + 1         # the jump is spread evenly over m + 1 steps


# ---- robustness ----------------------------------------------------------------------------------------------------------------
def test_out_of_range_index_gives_a_nan_row_and_touches_nothing_else(small):
    c = _clips(small, 'tail')
    plan = c['plan']
    N = plan[5]
    good = _launch(small, c['rep_norm'], c['transf'], 'bc1t', plan, True, True, True)
    fa, ta, fb, tb, alpha = (np.array(v) for v in plan[:5])
    shared = np.flatnonzero(fb >= 0)
    bad_a = {2: (4, 0), 5: (-1, 3), 17: (1, ROWS), 38: (2 ** 31 - 1, 2 ** 31 - 1), int(shared[0]): (0, -1)}
    bad_b = {int(shared[1]): (4, 0), int(shared[3]): (1, ROWS), int(shared[4]): (2, -1), int(shared[-1]): (2 ** 31 - 1, -2 ** 31)}
    for n, (cc, t) in bad_a.items():
        fa[n], ta[n] = cc, t
    for n, (cc, t) in bad_b.items():
        fb[n], tb[n] = cc, t
    tb[7] = 2 ** 31 - 1                                               # frame 7 has one candidate: its b row is not looked at
    fb[8] = -7                                                        # any negative clip_b means "one candidate"
    got = _launch(small, c['rep_norm'], c['transf'], 'bc1t', (fa, ta, fb, tb, alpha), True, True, True)
    rows = sorted(set(bad_a) | set(bad_b))
    rest = [n for n in range(N) if n not in rows]
    assert len(rows) == 9
    for g, w in zip(got, good):
        assert torch.isnan(g[rows]).all() and torch.equal(g[rest], w[rest])
    want = BR.export_blend(c['rep_norm'], (fa, ta, fb, tb, alpha), small['pelvis'], transf=c['transf'], rigid=small['rigid'],
                           mean=small['mean'], std=small['std'])
    for g, w in zip(got, want):
        assert np.array_equal(np.isnan(g.cpu().numpy()), np.isnan(w))


def test_no_frames_no_launch(small):
    from rohm_amd import _lib, ops
    c = _clips(small, 'regular')
    empty = np.zeros(0, np.int32)
    _lib.profile_start()
    out = _launch(small, c['rep'], c['transf'], 'btc', (empty, empty, empty, empty, np.zeros(0)), False, True, False)
    rows = _lib.profile_stop()
    assert 'export_smplx_blend' not in rows, rows
    assert [tuple(t.shape) for t in out] == [(0, 79), (0, 4), (0, 23)]
    _lib.profile_start()
    params, contact, disagree = _launch(small, c['rep'], c['transf'], 'btc', c['plan'], False, True, False, want_contact=False,
                                        want_disagree=False)
    assert _lib.profile_stop()['export_smplx_blend']['launches'] == 1 and contact is None and disagree is None
    assert torch.equal(params, _launch(small, c['rep'], c['transf'], 'btc', c['plan'], False, True, False)[0])
    i32 = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(_lib.RohmHipError):
        ops.export_smplx_blend(small['handle'], torch.zeros(3, ROWS, 294), 'btc', i32, i32, i32, i32, torch.zeros(1, dtype=torch.float64))
    with pytest.raises(ValueError, match='alpha'):
        ops.export_smplx_blend(small['handle'], _dev(c['rep']), 'btc', *[_dev(empty)] * 4, _dev(np.zeros(0, np.float32)))
    with pytest.raises(ValueError, match='frame_clip_b'):
        ops.export_smplx_blend(small['handle'], _dev(c['rep']), 'btc', *[_dev(empty)] * 3, _dev(np.zeros(0, np.int64)), _dev(np.zeros(0)))


def test_stale_output_buffers_do_not_show(small):
    """Output buffers that held something before (tests/stale_memory.py's poisoning allocators) give the bits of zeroed ones:
    every element of params, contact and disagree is written, NaN rows and one-candidate rows included."""
    c = _clips(small, 'heavy')
    fa, ta, fb, tb, alpha = (np.array(v) for v in c['plan'][:5])
    fa[3], fb[9] = 9, 9                                               # a NaN row from either side
    plan = (fa, ta, fb, tb, alpha)
    with SM.poison(SM.ZEROS):
        want = _launch(small, c['rep_norm'], c['transf'], 'bc1t', plan, True, True, True)
    assert torch.isnan(want[0][3]).all() and torch.isnan(want[2][9, :23]).all() and not want[2][0].any()
    for name, word in sorted(SM.PATTERNS.items()):
        with SM.poison(word):
            got = _launch(small, c['rep_norm'], c['transf'], 'bc1t', plan, True, True, True)
        for g, w, what in zip(got, want, ('params', 'contact', 'disagree')):
            assert SM.first_difference(g, w) is None, (name, what, SM.first_difference(g, w))


# ---- the interface ---------------------------------------------------------------------------------------------------------------
def test_export_params_blend_plan_and_mean_betas(small):
    from rohm_amd.export import export_params, plan_blend
    c = _clips(small, 'tail')
    plan = c['plan']
    res = export_params(c['rep_norm'], c['transf'], small['layer'], stats=(small['mean'], small['std']), frame='camera',
                        cam2world=small['cam2world'], plan=plan[:5])
    direct = _launch(small, c['rep_norm'], c['transf'], 'btc', plan, True, True, True)
    assert torch.equal(res.params79, direct[0]) and torch.equal(res.contact, direct[1]) and torch.equal(res.disagree, direct[2])
    assert res.frame_clip_b.cpu().tolist() == plan[2].tolist() and torch.equal(res.alpha.cpu(), torch.from_numpy(plan[4]))
    assert tuple(res.joints.shape) == (39, 22, 3) and res.coordinate_frame == 'camera'
    with pytest.raises(ValueError, match='blend'):
        export_params(c['rep'], c['transf'], small['layer'], keep='blend', plan=plan[:2])
    with pytest.raises(ValueError, match='keep'):
        export_params(c['rep'], c['transf'], small['layer'], keep='both')
    # regular windows through keep='blend' are plan_blend of arange(C) * stride
    reg = _clips(small, 'regular')
    a = export_params(reg['rep'], reg['transf'], small['layer'], clip_len=17, overlap_len=7, keep='blend')
    b = export_params(reg['rep'], reg['transf'], small['layer'], plan=plan_blend([0, 10, 20], ROWS)[:5])
    assert torch.equal(a.params79, b.params79) and torch.equal(a.disagree, b.disagree) and len(a) == 36
    # betas='mean': one shape, the mean over the candidate-a rows, seen by the kernel (pelvis offset and translation follow)
    per_frame = export_params(reg['rep'], reg['transf'], small['layer'], clip_len=17, overlap_len=7, keep='blend')
    mean = export_params(reg['rep'], reg['transf'], small['layer'], clip_len=17, overlap_len=7, keep='blend', betas='mean')
    rows_a = reg['rep'][reg['plan'][0], reg['plan'][1], 280:290].astype(np.float64).mean(axis=0).astype(np.float32)
    assert float((mean.betas - mean.betas[:1]).abs().max()) == 0.0
    assert np.abs(mean.betas[0].cpu().numpy() - rows_a).max() < 1e-6
    assert torch.equal(mean.global_orient, per_frame.global_orient) and not torch.equal(mean.transl, per_frame.transl)
    den = reg['rep'].copy()
    den[:, :, 280:290] = mean.betas[0].float().cpu().numpy()
    want = BR.export_blend(den, reg['plan'], small['pelvis'], transf=reg['transf'])[0]
    assert np.abs(mean.params79.cpu().numpy()[:, 3:16] - want[:, 3:16]).max() <= KERNEL_BAR


# ---- end to end: the track driver's pickle through the command line ---------------------------------------------------------------
TODAYS_KEYS = {'global_orient', 'transl', 'betas', 'body_pose', 'joints', 'foot_contact', 'frame_names', 'frame_clip', 'coordinate_frame',
               'gender', 'times', 'gap'}
BLEND_KEYS = {'frame_clip_b', 'blend_alpha', 'seam_angle', 'seam_dist'}


@pytest.fixture(scope='module')
def driven(scene, body_dir, tmp_path_factory):  # noqa: F811
    """One run of `drivers track` on the 25 fps track with a hole of tests/test_gpu_track.py, windows that share 8 frames."""
    from rohm_amd.drivers.__main__ import main
    a, paths, ck = scene
    tmp = tmp_path_factory.mktemp('blend_e2e')
    track = str(tmp / 'cam25.npz')
    np.savez(track, **holed_25fps_track(a, 50, 40, [0, 17, 18, 19, 20, 21]))
    out = main(['track', '--track', track, '--window_size', '8'] + _common(body_dir, ck, str(tmp / 'res'), seed='6'))
    return str(a['recording_name']), out['path'], tmp


@pytest.mark.parametrize('times', ['30fps', 'source'])
def test_command_line_blends_a_track(driven, body_dir, times, capsys):  # noqa: F811
    from rohm_amd.export import main as export_main
    from rohm_amd.export import plan_blend
    rec, pkl, tmp = driven
    got = _load(pkl)
    assert got['clip_starts'].tolist() == [0, 9, 18, 27, 29] and got['motion_repr_rec_list'].shape[1] == 15
    common = ['--dataset', 'track', '--saved_data_path', pkl, '--body_model_path', body_dir, '--clip_len', '17', '--times', times,
              '--frame', 'camera']
    z = {}
    for keep in ('first', 'blend', 'default'):
        capsys.readouterr()
        argv = common + ['--out', str(tmp / f'{times}_{keep}')] + ([] if keep == 'default' else ['--keep', keep])
        assert export_main(argv) == 0
        text = capsys.readouterr().out
        assert ('seams blended' in text) == (keep == 'blend')
        if keep == 'blend':
            assert f'{rec}: 4 seams blended, largest seam_angle' in text
        z[keep] = dict(np.load(str(tmp / f'{times}_{keep}' / rec / 'smplx_params.npz')))
    # without --keep blend: exactly today's keys and arrays, whether --keep first is given or not
    assert set(z['first']) == set(z['default']) == TODAYS_KEYS and set(z['blend']) == TODAYS_KEYS | BLEND_KEYS
    for k in TODAYS_KEYS:
        assert z['first'][k].dtype == z['default'][k].dtype and np.array_equal(z['first'][k], z['default'][k]), k
    n = len(z['first']['transl'])
    assert n == (44 if times == '30fps' else 39)
    assert all(len(z['blend'][k]) == n for k in ('transl', 'global_orient', 'joints', 'frame_clip_b', 'blend_alpha', 'seam_angle', 'seam_dist'))
    for k in ('frame_names', 'times', 'gap'):
        assert np.array_equal(z['blend'][k], z['first'][k]), k
    # rows outside the seams are the 'first' export's bits
    plan = plan_blend(got['clip_starts'], 15)
    seam30 = plan[2] >= 0
    assert plan[5] == 44 and seam30.sum() == 6 + 6 + 6 + 9
    if times == '30fps':
        outside = ~seam30
        assert np.array_equal(z['blend']['frame_clip_b'], plan[2]) and np.array_equal(z['blend']['blend_alpha'], plan[4])
    else:
        i0, i1, _, _ = TR.brackets(got['times_dst'][:44], np.ones(44, bool), z['blend']['times'], 1.5 / 30.0)
        outside = ~seam30[i0] & ~seam30[i1]                          # both brackets of the source time outside every seam
        assert np.array_equal(z['blend']['frame_clip_b'], plan[2][i0])
    assert 0 < outside.sum() < n
    for k in ('global_orient', 'transl', 'betas', 'body_pose', 'joints', 'foot_contact'):
        assert np.array_equal(z['blend'][k][outside], z['first'][k][outside]), k
        assert np.isfinite(z['blend'][k]).all()
    assert not np.array_equal(z['blend']['transl'][~outside], z['first']['transl'][~outside])
    single = z['blend']['frame_clip_b'] < 0
    assert not z['blend']['seam_angle'][single].any() and not z['blend']['seam_dist'][single].any()
    assert (z['blend']['seam_angle'][~single] > 0).all() and (z['blend']['seam_dist'][~single] > 0).all()
    assert ((z['blend']['blend_alpha'] > 0) == ~single).all() and (z['blend']['blend_alpha'] < 1).all()
