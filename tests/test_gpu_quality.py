"""GPU: scoring a reconstructed track without ground truth -- `rohm_track_quality` and `rohm_floor_clearance` (csrc/quality.hip)
against their float64 restatement (tests/quality_ref.py, held to hand-computable cases in tests/test_quality_ref.py), the
skating / acceleration / penetration columns pinned to the reference-pinned `rohm_scene_metrics`, and `score_recording` /
`python -m rohm_amd.quality` end to end on the fixtures of tests/test_gpu_track.py.

Kernel and restatement are both float64 on the same float32 inputs and differ by operation order and fma contraction only.
Bars: flags and counts equal (the inputs keep every compared quantity at least `MARGIN` away from its threshold, asserted on
the host); real columns within 1e-12 of the column's largest magnitude, the bar of the project's other float64 kernels
(profiles/track_parity.json).  The measured maxima go to profiles/quality_parity.json."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

import quality_ref as QR
import track_ref as TR
import video_tree as VT
from rohm_amd.utils import synth

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-12
# The issue asks for 1e-6 between the restatement's speeds / heights and every threshold.  The same inputs are also scored by
# rohm_scene_metrics, which computes them in float32: a speed is 30 * |difference of two coordinates below 4 m|, off by at most
# 30 * 3 * 2.4e-7 = 2.2e-5 m/s, a height by 2.4e-7 m.  1e-4 covers both.
MARGIN = 1e-4
REAL_COLS, FLAG_COLS = (0, 1, 4, 5, 6, 7), (2, 3, 8, 9)
COUNT_TOT, SUM_TOT = (0, 2, 4, 5, 7, 8, 10, 12, 14), (1, 3, 6, 9, 11, 13)
PARITY = {}


def _record(key, value):
    path = os.path.join(ROOT, 'profiles', 'quality_parity.json')
    PARITY[key] = max(float(value), PARITY.get(key, 0.0))
    try:
        with open(path) as f:
            data = json.load(f)
    except (OSError, ValueError):
        data = {}
    data['bar'] = BAR
    data.setdefault('gpu', {}).update(PARITY)
    try:
        with open(path, 'w') as f:
            json.dump(data, f, indent=1, sort_keys=True)
            f.write('\n')
    except OSError:
        pass


def _layer():
    from rohm_amd.body_model import SMPLXLayer
    return SMPLXLayer.from_tensors(synth.synthetic_smplx_tensors(0)).to(DEV)


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)            # a copy: the shared inputs are read-only


# ---- inputs ----------------------------------------------------------------------------------------------------------------
SCENE2CAM = np.array([[1.0, 0.0, 0.0, 0.05], [0.0, 0.0, -1.0, 1.1], [0.0, 1.0, 0.0, 3.0], [0.0, 0.0, 0.0, 1.0]])      # looks along scene y
CAM = (1060.53, 1060.38, 951.3, 536.77)
GROUND = -0.05
SIZES = (1, 2, 3, 50, 1031)


def _off(g, lo, hi, avoid, eps, size):
    """uniform in [lo, hi) but at least eps away from every value of `avoid`."""
    v = g.uniform(lo, hi, size=size)
    for a in avoid:
        near = np.abs(v - a) < eps
        v = np.where(near, a + np.where(v >= a, eps, -eps) * 2, v)
    return v


def make_inputs(N, seed, up_axis=2):
    """A random track about 1 m in size (z up; `up_axis=1` exchanges y and z afterwards), built so that the flags are mixed and
    far from their thresholds: in about 40 % of the frames all four foot joints are low and fast (they skate), elsewhere each
    foot is slow, fast, low or high at random; toes reach under the floor.  Returns a dict of host arrays."""
    g = np.random.Generator(np.random.PCG64(seed))
    j = g.uniform(-0.5, 0.5, size=(N, 22, 3))
    j[..., 2] += 1.0
    skating = g.uniform(size=N) < 0.4
    speed = np.where(g.uniform(size=(N, 4)) < 0.5, g.uniform(0.02, 0.08, size=(N, 4)), g.uniform(0.15, 0.6, size=(N, 4)))
    speed = np.where(skating[:, None], g.uniform(0.15, 0.6, size=(N, 4)), speed)
    ang = g.uniform(0, 2 * np.pi, size=(N, 4))
    step = np.stack([np.cos(ang), np.sin(ang)], axis=-1) * (speed / 30.0)[..., None]
    xy = g.uniform(-0.3, 0.3, size=(1, 4, 2)) + np.concatenate([np.zeros((1, 4, 2)), np.cumsum(step[:-1], axis=0)], axis=0)
    hmax = np.asarray(QR.FOOT_HMAX)
    h = np.stack([_off(g, -0.12, 0.3, (hmax[k], QR.PENE_DEPTH), 2e-3, N) for k in range(4)], axis=1)
    low = np.stack([_off(g, -0.12, 0.09, (QR.PENE_DEPTH,), 2e-3, N) for k in range(4)], axis=1)
    h = np.where(skating[:, None], low, h)
    j[:, list(QR.FOOT), 0:2] = xy
    j[:, list(QR.FOOT), 2] = h + GROUND
    if N > 0:
        j[N // 2, 15] = (0.1, -4.5, 1.0)                                   # behind the camera: Z = y + 3 < 0
    j = j.astype(np.float32)
    uv, Z, _ = QR.project(j, SCENE2CAM, *CAM)
    kp = np.concatenate([uv + g.normal(0, 4.0, size=uv.shape), g.uniform(0.05, 1.0, size=(N, 22, 1))], axis=-1)
    kp[N // 2, 15] = (300.0, 200.0, 0.9)                                   # confident, but its joint is behind the camera
    for t in (1, 7, 8):
        if t < N:
            kp[t] = 0.0                                                    # nobody detected
    mask = (g.uniform(size=(N, 22)) > 0.35).astype(np.float32)
    mask[0] = 1.0
    if N > 1:
        mask[N - 1] = 0.0
    gap = (g.uniform(size=N) < 0.3).astype(np.uint8)
    ref = (j + g.normal(0, 0.03, size=j.shape)).astype(np.float32)
    d = dict(joints=j, keypoints=kp.astype(np.float32), joints_ref=ref, mask_ref=mask, gap=gap)
    if up_axis == 1:
        d['joints'], d['joints_ref'] = j[..., [0, 2, 1]].copy(), ref[..., [0, 2, 1]].copy()
    return d


def _scene2cam(up_axis):
    return SCENE2CAM if up_axis == 2 else SCENE2CAM[:, [0, 2, 1, 3]]


def run_kernel(d, up_axis=2, floor=True, camera=True, ref=True, mask=True, gap=True, conf_min=0.2):
    from rohm_amd.quality import track_quality
    kw = {}
    if camera:
        kw.update(keypoints=_dev(d['keypoints']), scene2cam=_scene2cam(up_axis), focal=CAM[:2], center=CAM[2:])
    return track_quality(_dev(d['joints']), 30.0, 'z' if up_axis == 2 else 'y', GROUND if floor else None, conf_min=conf_min,
                         joints_ref=_dev(d['joints_ref']) if ref else None, mask_ref=_dev(d['mask_ref']) if mask else None,
                         gap=_dev(d['gap']) if gap else None, **kw)


def run_ref(d, up_axis=2, floor=True, camera=True, ref=True, mask=True, gap=True, conf_min=0.2):
    cam = dict(scene2cam=_scene2cam(up_axis), fx=CAM[0], fy=CAM[1], cx=CAM[2], cy=CAM[3], keypoints=d['keypoints']) if camera else {}
    return QR.track_quality(d['joints'], 30.0, up_axis, floor, GROUND, conf_min=conf_min, joints_ref=d['joints_ref'] if ref else None,
                            mask_ref=d['mask_ref'] if mask else None, gap=d['gap'] if gap else None, **cam)


REFS = {}


def inputs_and_ref(N, up_axis=2):
    """The inputs of size N with the restatement's rows and totals, computed once and shared (nobody writes to them)."""
    if (N, up_axis) not in REFS:
        d = make_inputs(N, 100 + N, up_axis)
        margin = QR.threshold_margin(d['joints'], 30.0, up_axis, GROUND, _scene2cam(up_axis))
        assert margin >= MARGIN, margin
        REFS[N, up_axis] = (d, ) + run_ref(d, up_axis)
        for a in list(d.values()) + list(REFS[N, up_axis][1:]):
            a.setflags(write=False)
    return REFS[N, up_axis]


def compare(q, rows_want, tot_want, tag):
    rows, tot = q.rows.cpu().numpy(), q.totals
    assert rows.shape == rows_want.shape and rows.dtype == np.float64 and tot.shape == (2, 15)
    assert np.array_equal(np.isnan(rows), np.isnan(rows_want))
    for c in FLAG_COLS:
        assert np.array_equal(rows[:, c], rows_want[:, c], equal_nan=True), (tag, c)
    worst = 0.0
    for c in REAL_COLS:
        ok = ~np.isnan(rows_want[:, c])
        if ok.any():
            rel = np.abs(rows[ok, c] - rows_want[ok, c]).max() / max(np.abs(rows_want[ok, c]).max(), 1e-300)
            print(f'{tag}: column {c} ({QR.COLS[c]}) max |kernel - restatement| / max |column| = {rel:.3e} (bar {BAR:.0e})')
            _record(f'{tag}_{QR.COLS[c]}_max_rel', rel)
            worst = max(worst, rel)
    for c in COUNT_TOT:
        assert np.array_equal(tot[:, c], tot_want[:, c]), (tag, 'totals', c, tot[:, c], tot_want[:, c])
    assert np.array_equal(np.isnan(tot), np.isnan(tot_want))
    for c in SUM_TOT:
        ok = ~np.isnan(tot_want[:, c])
        rel = (np.abs(tot[ok, c] - tot_want[ok, c]) / np.maximum(np.abs(tot_want[ok, c]), 1e-300)).max() if ok.any() else 0.0
        rel = 0.0 if (tot_want[ok, c] == tot[ok, c]).all() else rel
        print(f'{tag}: totals column {c} max relative difference {rel:.3e} (bar {BAR:.0e})')
        _record(f'{tag}_totals_{c}_max_rel', rel)
        worst = max(worst, rel)
    assert worst <= BAR, (tag, worst)


# ---- 1. kernel against restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', SIZES)
def test_kernel_matches_the_restatement(N):
    d, rows_want, tot_want = inputs_and_ref(N)
    assert np.isnan(rows_want[-1, 3]) and np.isnan(rows_want[-2:, 4]).all()                    # the NaN tails
    if N >= 50:
        assert 0 < np.nansum(rows_want[:, 3]) < N - 1 and 0 < tot_want[:, 8].sum() < tot_want[:, 10].sum()      # mixed flags
        assert np.isnan(rows_want[1, 0]) and rows_want[1, 2] == 0 and (rows_want[:, 2] < 22).any() and tot_want[1, 0] > 0
        assert rows_want[0, 8] == 22 and np.isnan(rows_want[0, 7]) and rows_want[-1, 8] == 0 and np.isnan(rows_want[-1, 6])
    compare(run_kernel(d), rows_want, tot_want, f'n{N}')


def test_kernel_options():
    """y up, and every optional input left out in turn: no floor, no camera, no input track, no mask, no gap."""
    d, rows_want, tot_want = inputs_and_ref(50, up_axis=1)
    compare(run_kernel(d, up_axis=1), rows_want, tot_want, 'n50_y_up')
    d = inputs_and_ref(50)[0]
    for off in ('floor', 'camera', 'ref', 'mask', 'gap'):
        q = run_kernel(d, **{off: False})
        rows_want, tot_want = run_ref(d, **{off: False})
        compare(q, rows_want, tot_want, 'n50_no_' + off)
        rows = q.rows.cpu().numpy()
        nan_cols = {'floor': (3, 5), 'camera': (0, 1), 'ref': (6, 7)}.get(off, ())
        assert all(np.isnan(rows[:, c]).all() for c in nan_cols)
        if off == 'mask':
            assert (rows[:, 8] == 22).all() and np.isnan(rows[:, 7]).all()
        if off == 'gap':
            assert not rows[:, 9].any() and q.totals[1, 0] == 0 and q.totals[0, 0] == 50
    from rohm_amd.quality import track_quality
    empty = track_quality(torch.empty(0, 22, 3, device=DEV), floor_height=0.0)
    assert tuple(empty.rows.shape) == (0, 10) and empty.totals[:, 0].tolist() == [0, 0] and np.isnan(empty.summary()['all']['acc'])


def test_kernel_refuses_bad_arguments():
    from rohm_amd import _lib
    from rohm_amd.quality import floor_clearance, track_quality
    j = torch.zeros(4, 22, 3, device=DEV)
    with pytest.raises(ValueError, match=r'\[N, 22, 3\]'):
        track_quality(j[:, :21])
    with pytest.raises(ValueError, match='keypoints must be'):
        track_quality(j, keypoints=j[:3], scene2cam=np.eye(4), focal=(1, 1), center=(0, 0))
    with pytest.raises(ValueError, match='together'):
        track_quality(j, keypoints=j)
    with pytest.raises(ValueError, match='up_axis'):
        track_quality(j, up_axis='x')
    with pytest.raises(_lib.RohmHipError, match='no CPU fallback'):
        track_quality(j, joints_ref=j.cpu())
    with pytest.raises(TypeError):
        floor_clearance(np.zeros((1, 3, 3)), 'z', 0.0)
    with pytest.raises(ValueError, match='verts must be'):
        floor_clearance(j[:, :, :2], 'z', 0.0)
    lib, stream = _lib.lib(), _lib.stream_ptr(torch.device(DEV))
    rows, tot = torch.empty(4, 10, device=DEV, dtype=torch.float64), torch.empty(2, 15, device=DEV, dtype=torch.float64)
    m = torch.eye(4, device=DEV, dtype=torch.float64)

    def call(N=4, fps=30.0, up=2, s2c=None, kp=None, rows_ptr=rows.data_ptr()):
        return lib.rohm_track_quality(j.data_ptr(), N, fps, up, 1, 0.0, s2c, 1.0, 1.0, 0.0, 0.0, kp, 0.2, None, None, None, rows_ptr,
                                      tot.data_ptr(), stream)
    assert call() == 0 and call(N=0, rows_ptr=None) == 0
    assert call(N=-1) == -1 and b'N must be' in lib.rohm_last_error()
    assert call(up=0) == -1 and b'up_axis' in lib.rohm_last_error()
    assert call(fps=0.0) == -1 and b'fps' in lib.rohm_last_error()
    assert call(s2c=m.data_ptr()) == -1 and b'go together' in lib.rohm_last_error()
    assert call(rows_ptr=None) == -1 and b'null' in lib.rohm_last_error()
    assert lib.rohm_floor_clearance(j.data_ptr(), 1, 0, 2, 0.0, 0.05, rows.data_ptr(), stream) == -1 and b'V >= 1' in lib.rohm_last_error()
    torch.cuda.synchronize()


# ---- 2. the same input twice; totals from rows -----------------------------------------------------------------------------------
@pytest.mark.parametrize('N', (50, 1031))
def test_same_input_same_bits_and_totals_are_the_rows(N):
    d = inputs_and_ref(N)[0]
    a, b = run_kernel(d), run_kernel(d)
    assert torch.equal(a.rows.view(torch.int64), b.rows.view(torch.int64))
    assert a.totals.tobytes() == b.totals.tobytes()
    toe_d = d['joints'][:, list(QR.TOES), 2].astype(np.float64) - float(np.float32(GROUND))
    want = QR.totals_from(a.rows.cpu().numpy(), toe_d)
    for c in COUNT_TOT:
        assert np.array_equal(a.totals[:, c], want[:, c]), c
    for c in SUM_TOT:
        rel = np.abs(a.totals[:, c] - want[:, c]) / np.maximum(np.abs(want[:, c]), 1e-300)
        print(f'n{N}: totals column {c} against the host sum of the rows: {rel.max():.3e} (bar {BAR:.0e})')
        _record(f'n{N}_totals_from_rows_{c}_max_rel', rel.max())
        assert (rel <= BAR).all(), (c, rel)


# ---- 3. NaN containment ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('joint', (10, 3))
def test_a_nan_joint_stays_where_it_is_read(joint):
    d = dict(inputs_and_ref(50)[0])
    t = 20
    d['keypoints'] = d['keypoints'].copy()
    d['keypoints'][t, joint, 2] = 0.9
    d['mask_ref'] = d['mask_ref'].copy()
    d['mask_ref'][t, joint] = 1.0
    base = run_kernel(d).rows.cpu().numpy()
    d['joints'] = d['joints'].copy()
    d['joints'][t, joint] = np.nan
    q = run_kernel(d)
    rows = q.rows.cpu().numpy()
    want = np.zeros(rows.shape, bool)
    want[[t - 2, t - 1, t], 4] = True
    want[t, [0, 1, 2, 6]] = True
    if joint in QR.FOOT:
        want[[t - 1, t], 3] = True
        want[t, 5] = True
    assert np.isnan(rows[want]).all() and not np.isnan(base[want]).any()
    assert np.array_equal(rows[~want].view(np.int64), base[~want].view(np.int64))                # every other element: the same bits
    rows_want, tot_want = run_ref(d)
    assert np.array_equal(np.isnan(rows), np.isnan(rows_want))
    for c in COUNT_TOT:
        assert np.array_equal(q.totals[:, c], tot_want[:, c]), c


# ---- 4. pinned to the reference-pinned kernel -----------------------------------------------------------------------------------------
def test_pinned_to_scene_metrics():
    from rohm_amd.evaluation import scene_metrics
    T = 50
    d, rows_want, tot_want = inputs_and_ref(T)
    q = run_kernel(d, camera=False, ref=False, mask=False)
    s = scene_metrics(_dev(d['joints'])[None], torch.eye(4, device=DEV)[None], GROUND, 'prox').sums[0]
    tot = q.totals.sum(axis=0)
    assert tot[5] == T - 1 and tot[7] == T - 2 and tot[10] == 2 * T
    assert tot[4] == s[0] and 0 < s[0] < T - 1, (tot[4], s[0])                               # skating pairs
    assert tot[8] == s[3] and 0 < s[3] < 2 * T, (tot[8], s[3])                               # toe entries below -0.05 m
    acc = np.nansum(q.rows.cpu().numpy()[:, 4]) * 22
    print(f'sum |acc|: {acc:.6f} against {s[1]:.6f} (float32 second differences), bar {(T - 2) * 22 * 2e-3:.3f} m/s^2')
    assert abs(acc - s[1]) <= (T - 2) * 22 * 2e-3
    print(f'penetration sum: {tot[9]:.9f} against {s[4]:.9f}')
    assert abs(tot[9] - s[4]) <= 1e-6 * abs(s[4]) and s[4] < 0


# ---- 6. floor clearance -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('V', (1, 7, 10475))
def test_floor_clearance_matches_numpy(V):
    from rohm_amd.quality import floor_clearance
    g = np.random.Generator(np.random.PCG64(V))
    v = g.uniform(-0.3, 1.7, size=(3, V, 3)).astype(np.float32)
    if V > 1:
        i, k = sorted(g.choice(V, size=2, replace=False).tolist())
        v[1, [i, k], 2] = np.float32(-0.4)                                                        # a tie for the lowest: index i
        v[2, [i, k], 1] = np.float32(-0.4)
    for up, axis in (('z', 2), ('y', 1)):
        got = floor_clearance(_dev(v), up, -0.02, 0.05).cpu().numpy()
        want = QR.floor_clearance(v, axis, -0.02, 0.05)
        assert got.dtype == np.float64 and np.array_equal(got, want), (up, got, want)
        if V > 1:
            assert got[3 - axis, 1] == i and want[3 - axis, 2] >= 2                             # the tie is in frame 1 (z) / 2 (y)
    again = floor_clearance(_dev(v), 'z', -0.02, 0.05).cpu().numpy()
    assert again.tobytes() == QR.floor_clearance(v, 2, -0.02, 0.05).tobytes()
    if V == 7:
        v[0, 3, 2] = np.inf
        got = floor_clearance(_dev(v), 'z', -0.02).cpu().numpy()
        assert np.array_equal(got, QR.floor_clearance(v, 2, -0.02), equal_nan=True) and np.isnan(got[0, 0]) and got[0, 1] == -1
        assert tuple(floor_clearance(_dev(v[:0]), 'z', 0.0).shape) == (0, 3)


def test_floor_clearance_over_vertex_chunks():
    from rohm_amd.export import ExportResult, _joints, _vertex_chunks
    from rohm_amd.body_model import native_for
    from rohm_amd.quality import floor_clearance
    layer = _layer()
    n = 300
    g = np.random.Generator(np.random.PCG64(11))
    t = np.arange(n) / 30.0
    params = 0.45 * np.sin(2 * np.pi * g.uniform(0.05, 0.4, size=79) * t[:, None] + g.uniform(0, 2 * np.pi, size=79))      # smooth, < 0.8 rad
    params[:, 3:6] += (0.0, 0.0, 1.0)
    params[:, 6:16] = g.standard_normal(10) * 0.3
    params = _dev(params)
    res = ExportResult(params, None, None, None, None, 'scene')
    res.joints = _joints(native_for(layer, torch.device(DEV)), res.pose_f32(), res.betas.float().contiguous(), res.transl.float().contiguous())
    parts, seen = [], []
    for sel, verts in _vertex_chunks(res, layer):
        assert verts.shape[0] <= 256
        parts.append(floor_clearance(verts, 'z', 0.0))
        seen.append(verts[:, :, 2].min(dim=1).values.double())
    clear = torch.cat(parts).cpu().numpy()
    assert clear.shape == (n, 3) and np.array_equal(clear[:, 0], torch.cat(seen).cpu().numpy())
    toe = res.joints[:, list(QR.TOES), 2].min(dim=1).values.double().cpu().numpy()
    print(f'lowest vertex against the lower toe joint: {np.max(clear[:, 0] - toe):.4f} m at most above it (bound 0.2)')
    assert (clear[:, 0] <= toe + 0.2).all()


# ---- fixtures of tests/test_gpu_track.py (own copies of the small helpers) -------------------------------------------------------------
def _synthetic_arrays(dataset, n, seed):
    keep = VT.N_FRAMES
    VT.N_FRAMES = n
    try:
        return VT.synthetic_tree_arrays(dataset, seed=seed)
    finally:
        VT.N_FRAMES = keep


@pytest.fixture(scope='module')
def body_dir(tmp_path_factory):
    """SMPLX_NEUTRAL.npz in the released layout from the synthetic model."""
    t = synth.synthetic_smplx_tensors(0)
    V = t['v_template'].shape[0]
    kt = np.stack([np.array(synth.SMPLX_PARENTS), np.arange(55)]).astype(np.int64)
    kt[0, 0] = 2 ** 32 - 1
    d = tmp_path_factory.mktemp('body')
    np.savez(str(d / 'SMPLX_NEUTRAL.npz'), v_template=t['v_template'].numpy(), shapedirs=t['shapedirs'].numpy(),
             posedirs=t['posedirs'].numpy().T.reshape(V, 3, 486), J_regressor=t['J_regressor'].numpy(), kintree_table=kt,
             weights=t['lbs_weights'].numpy(), f=np.zeros((4, 3), np.int64))
    return str(d)


def _common(body_dir, ck, save_root, seed='4'):
    return ['--body_model_path', body_dir, '--model_path_posenet', ck['posenet'], '--model_path_trajnet', ck['trajnet'],
            '--model_path_trajnet_control', ck['control'], '--diffusion_steps_posenet', '6', '--diffusion_steps_trajnet', '4',
            '--sample_iter', '2', '--save_root', save_root, '--seed', seed, '--clip_len', '17', '--batch_size', '2']


def _load(path):
    with open(path, 'rb') as f:
        return pickle.load(f)


# The checkpoints are random, so the "reconstruction" is a body somewhere within a few metres of the input (with the body 3.7 m
# from the camera it was measured between 1 m behind the camera and 3 m in front of it).  A residual needs joints in front of the
# camera: the body stands 10 m away, where such a reconstruction stays in view and the projections are still about 1e3 px.
CAMERA_DEPTH = 10.0


def self_consistent_track(a, floor_height=-0.05):
    """The 50-frame synthetic PROX recording as a track whose keypoints_2d [N, 22, 3] are the projections of its own FK joints
    (`rohm_smplx_joints` through `frames_to_world`) through its own cam2world and intrinsics -- the restatement's projection --
    with confidence 0.9.  The body is moved along the camera's axis until it is at least `CAMERA_DEPTH` in front of it."""
    from rohm_amd.data_loaders import frames
    d = {k: a['params'][:, lo:hi].astype(np.float32) for k, (lo, hi) in VT.PARAM_SLICES.items()}
    d.update(cam2world=a['cam2world'], fps=30.0, up_axis='z', focal_length=a['cam_f'], camera_center=a['cam_c'], floor_height=floor_height,
             frame_names=a['frame_names'], recording_name=str(a['recording_name']), mask_joint=np.ones((len(a['params']), 25), np.float32))
    scene2cam = np.linalg.inv(np.asarray(a['cam2world'], dtype=np.float64))
    layer = _layer()

    def depth():
        jw = frames.frames_to_world(layer, d, a['cam2world'], DEV)[0].cpu().numpy()
        return jw, QR.project(jw, scene2cam, *a['cam_f'], *a['cam_c'])
    jw, (uv, Z, _) = depth()
    d['transl'] = d['transl'] + np.float32([0.0, 0.0, max(0.0, np.ceil(CAMERA_DEPTH - Z.min()))])
    jw, (uv, Z, _) = depth()
    assert Z.min() >= CAMERA_DEPTH - 0.1
    d['keypoints_2d'] = np.concatenate([uv, np.full(uv.shape[:2] + (1,), 0.9)], axis=-1).astype(np.float32)
    return d


def holed_25fps(src, n30, n25, hole):
    """`src` (30 fps, n30 frames) resampled on the host to n25 frames at 25 fps, with the frames `hole` lost."""
    t30, t25 = np.arange(n30) / 30.0, np.arange(n25) / 25.0
    assert t25[-1] <= t30[-1]
    p = np.concatenate([src[k].astype(np.float64) for k in ('global_orient', 'transl', 'betas', 'body_pose')], axis=1)
    r = TR.resample(t30, np.ones(n30, bool), p, src['keypoints_2d'], None, t25, 1.0)
    valid = np.ones(n25, bool)
    valid[hole] = False
    out = dict(src, fps=25.0, keypoints_2d=r['keypoints'], mask_joint=np.ones((n25, 25), np.float32), valid=valid,
               frame_names=np.array(['cam_%04d' % i for i in range(n25)]))
    for k, (lo, hi) in (('global_orient', (0, 3)), ('transl', (3, 6)), ('betas', (6, 16)), ('body_pose', (16, 79))):
        out[k] = r['params'][:, lo:hi].astype(np.float32)
        out[k][hole] = np.nan
    return out


@pytest.fixture(scope='module')
def runs(tmp_path_factory, body_dir):
    """`drivers track` once on the self-consistent 30 fps track and once on its 25 fps version with a hole:
    {name: (track path, pickle path)}, shared by the tests below."""
    from rohm_amd.drivers.__main__ import main
    a = _synthetic_arrays('prox', 50, 3)
    root = tmp_path_factory.mktemp('quality')
    paths = VT.write_tree(str(root / 'tree'), 'prox', a)
    ck = {}
    for k, sd in (('posenet', synth.posenet_state_dict(0)), ('trajnet', synth.trajnet_state_dict(1, trajcontrol=False)),
                  ('control', synth.trajnet_state_dict(2, trajcontrol=True))):
        ck[k] = os.path.join(paths['logdir'], f'model_{k}.pt')
        torch.save(sd, ck[k])
    src = self_consistent_track(a)
    out = {}
    for name, track in (('walk30', src), ('cam25', holed_25fps(src, 50, 40, [0, 17, 18, 19, 20, 21]))):
        path = str(root / f'{name}.npz')
        np.savez(path, **track)
        out[name] = (path, main(['track', '--track', path] + _common(body_dir, ck, str(root / name), seed='6'))['path'])
    return out


# ---- 5. conventions end to end ------------------------------------------------------------------------------------------------------------
def test_score_recording_conventions(runs, body_dir):
    from rohm_amd.data_loaders.dataloader_video import _body_model
    from rohm_amd.quality import score_recording
    body = _body_model(body_dir, 'neutral', torch.device(DEV))
    track, pkl = runs['walk30']
    data = _load(pkl)
    s = score_recording(pkl, track, body, clip_len=17, device=DEV)
    assert set(s) == {'input', 'reconstruction'}
    rows_in, rows_rec = s['input'].rows_host(), s['reconstruction'].rows_host()
    n = len(rows_in)
    assert n == len(rows_rec) == int(data['clip_starts'][-1]) + 15 and data['clip_starts'].tolist() == [0, 15, 30, 33] and not data['gap'].any()
    print(f'input reproj_px on {n} frames: max {rows_in[:, 0].max():.3e} px (bar 1e-2), joints counted {rows_in[:, 2].min():.0f} .. 22')
    assert (rows_in[:, 2] == 22).all() and (rows_in[:, 0] < 1e-2).all()
    assert np.array_equal(rows_in[:, 9], data['gap'][:n]) and np.array_equal(rows_rec[:, 9], data['gap'][:n])
    assert np.isnan(rows_in[:, 6:8]).all() and (rows_in[:, 8] == 22).all()                      # the input has no joints_ref
    finite = np.isfinite(rows_rec)
    finite[-1, 3] = finite[-2:, 4] = True                                                       # the NaN tails
    finite[:, 7] = True                                                                         # nothing was occluded
    assert finite.all(), ('frames without a residual (nothing in front of the camera):', np.flatnonzero(np.isnan(rows_rec[:, 0])).tolist())
    assert np.isfinite(s['reconstruction'].totals[0, [1, 4, 6, 9, 11]]).all()
    assert np.array_equal(s['reconstruction'].times, data['times_dst'][:n])
    summ = s['reconstruction'].summary()
    assert summ['observed']['frames'] == n and summ['infilled']['frames'] == 0 and summ['all']['frames_reproj'] == n
    assert len(s['reconstruction'].lines()) == 9

    track, pkl = runs['cam25']
    data = _load(pkl)
    s = score_recording(pkl, track, body, vertices=True, device=DEV)
    n = len(s['input'])
    gap = np.asarray(data['gap'])[:n]
    assert n == int(data['clip_starts'][-1]) + 15 and 0 < gap.sum() < n
    for q in s.values():
        assert q.totals[1, 0] == gap.sum() and q.totals[1, 2] == 0 and q.totals[0, 0] == n - gap.sum()
        assert np.array_equal(q.rows_host()[:, 9], gap) and np.isnan(q.rows_host()[gap == 1, 0]).all()
        assert tuple(q.clearance.shape) == (n, 3) and 'mesh_lowest_mm' in q.summary()['all'] and len(q.lines()) == 11
    obs = s['input'].rows_host()[gap == 0]
    print(f'25 fps input reproj_px on observed frames: max {obs[:, 0].max():.3e} px')
    assert (obs[:, 2] == 22).all()
    # the in-filled frames carry no visibility: everything there is dev_occ
    rec = s['reconstruction'].rows_host()
    assert (rec[gap == 1, 8] == 0).all() and np.isnan(rec[gap == 1, 6]).all() and np.isfinite(rec[gap == 1, 7]).all()
    with pytest.raises(ValueError, match='not a track pickle'):
        score_recording({k: v for k, v in data.items() if k != 'clip_starts'}, track, body, device=DEV)


# ---- 7. the tool ---------------------------------------------------------------------------------------------------------------------------
def test_cli_round_trip_and_blend(runs, body_dir, tmp_path, capsys):
    from rohm_amd.export import main as export_main
    from rohm_amd.quality import COLUMNS, main
    track, pkl = runs['cam25']
    data = _load(pkl)
    js, rows = str(tmp_path / 'q.json'), str(tmp_path / 'rows.npz')
    assert main(['--saved_data_path', pkl, '--track', track, '--body_model_path', body_dir, '--clip_len', '17', '--json', js, '--rows', rows,
                 '--worst', '3']) == 0
    out = capsys.readouterr().out
    assert 'input' in out and 'reconstruction' in out and 'skating score:' in out and 'worst frame ranges' in out
    with open(js) as f:
        rep = json.load(f)
    rec_name = str(data['recording_name'])
    assert rep['columns'] == list(COLUMNS) and rep['keep'] == 'first' and list(rep['recordings']) == [rec_name]
    z = np.load(rows)
    n = int(data['clip_starts'][-1]) + 15
    assert z['rows_input'].shape == z['rows_reconstruction'].shape == (n, 10) and z['columns'].tolist() == list(COLUMNS)
    assert np.array_equal(z['times'], data['times_dst'][:n]) and np.array_equal(z['gap'], data['gap'][:n])
    summ = rep['recordings'][rec_name]['reconstruction']['summary']
    assert summ['infilled']['frames'] == int(z['gap'].sum()) and summ['all']['frames'] == n
    r = z['rows_reconstruction']
    assert np.isclose(summ['all']['acc'], np.nanmean(r[:, 4]), rtol=1e-12) and np.isclose(summ['observed']['reproj_px'],
                                                                                          np.nanmean(r[z['gap'] == 0, 0]), rtol=1e-12)
    worst = rep['recordings'][rec_name]['reconstruction']['worst']['accel']
    assert len(worst) <= 3 and worst[0][2] == np.nanmax(r[:, 4])
    # a blended export and a blended score have the same rows
    rows_b = str(tmp_path / 'rows_blend.npz')
    assert main(['--saved_data_path', pkl, '--track', track, '--body_model_path', body_dir, '--keep', 'blend', '--rows', rows_b, '--worst', '0']) == 0
    assert export_main(['--dataset', 'track', '--saved_data_path', pkl, '--body_model_path', body_dir, '--clip_len', '17', '--keep', 'blend',
                        '--times', '30fps', '--out', str(tmp_path / 'blend')]) == 0
    zb = np.load(rows_b)
    ex = np.load(str(tmp_path / 'blend' / rec_name / 'smplx_params.npz'))
    assert len(zb['rows_reconstruction']) == len(ex['transl']) and np.array_equal(zb['times'], ex['times']) and np.array_equal(zb['gap'], ex['gap'])
    # a track without keypoints and without a floor: NaN lines and a note, not an error
    bare = dict(np.load(track))
    for k in ('keypoints_2d', 'floor_height'):
        bare.pop(k)
    np.savez(str(tmp_path / 'bare.npz'), **bare)
    js2 = str(tmp_path / 'bare.json')
    assert main(['--saved_data_path', pkl, '--track', str(tmp_path / 'bare.npz'), '--body_model_path', body_dir, '--json', js2, '--vertices']) == 0
    out = capsys.readouterr().out
    assert out.count('note:') == 2 and 'keypoints_2d' in out and 'floor_height' in out
    with open(js2) as f:
        s2 = json.load(f)['recordings'][rec_name]['reconstruction']['summary']['all']
    assert all(np.isnan(s2[k]) for k in ('reproj_px', 'skating', 'ground_pene_freq')) and np.isfinite(s2['acc']) and np.isfinite(s2['dev_occ_mm'])
