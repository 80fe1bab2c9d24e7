"""GPU: multi-view triangulation -- `rohm_mv_triangulate` and `rohm_mv_residuals` (csrc/multiview.hip) against their float64
restatement (tests/multiview_ref.py, held to closed forms, central differences and planted points in tests/test_multiview_ref.py),
and `python -m rohm_amd.multiview` -> `python -m rohm_amd.fit` end to end with the synthetic body.

Shapes (`multiview_ref.GPU_CASES`), the smallest at which the kernel can go wrong: (V, N, J) = (2, 1, 22), one pair; (3, 1, 22);
(5, 3, 25); (16, 3, 22), 120 pairs: more than a wave of them; (4, 70, 25), 1 750 points: a multiple of neither 4, 16, 64 nor 256; (6, 3, 22) and (7, 3, 22), the two sides of the kernel's switch from
16 lanes per point to a wave per point.
Distortion off and on, `rigid` NULL and given, `keypoints_und` NULL and given; NaN and infinite coordinates, zero, negative and
NaN confidences, a frame nobody observes, a camera that looks away, two cameras at one place, planted outliers.

Bars.  Kernel and restatement are both float64 on the same float32 inputs; they differ by the order of sums of at most 16 terms,
by fused multiply-adds and by the device's sqrt and division, a few ulp.  `joints`: 1e-9 max(1, |X|) metres.  `report`'s rms and
sigma_m, and `resid`: 1e-9 relative.  That leaves about four decades of margin.  The inlier counts, the `inliers` masks, the
observed counts and the NaN pattern are EQUAL: that rests on the restatement's margins (no scored error within 1e-6 px of tau_px,
no pair within 1e-9 of the angle threshold, no cost gap below 1e-9 relative), which test_multiview_ref.py::test_margins_of_the_gpu_inputs
asserts on the CPU and `_margins` asserts here once per session.  `conf` and `keypoints_und` are float32 stores of float64 values:
a last-place difference can flip the rounding, so their bar is one float32 ulp.  Noise-free residuals: RESIDUAL_BAR_PX, the round
trip of five iterations (test_multiview_ref.ROUND_TRIP_PX = 1e-5 px) plus twice the float32 rounding of a detection (half a step
at 1024 px, 6.1e-5 px per coordinate, 8.7e-5 px in the norm): the fitted point moves by no more than the detections did.
End to end: 2 mm, the issue's bar.  The largest measured values go to profiles/multiview_parity.json."""
import json

import numpy as np
import pytest
import torch

import fit_ref as FR
import multiview_ref as MR
from rohm_amd.utils import synth

record = MR.record
pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BAR = 1e-9
RESIDUAL_BAR_PX = 1e-5 + 2 * 8.7e-5


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)            # a copy: the shared inputs are read-only


@pytest.fixture(scope='session')
def _margins():
    for name in MR.GPU_CASES:
        bad = MR.margins_ok(MR.build_case(name)['ref'])
        assert len(bad) == 0, f'{name}: points {bad[:5].tolist()} are within the margins the equalities rest on'


def run(case, **kw):
    from rohm_amd.multiview import triangulate
    t = triangulate(_dev(case['keypoints']), _dev(case['cams']), rigid=_dev(case['rigid']), want_undistorted=case['want_undistorted'], **kw)
    torch.cuda.synchronize()
    return t


def ulps32(a, b):
    """The distance of two float32 arrays in units of the last place (equal bit patterns, NaN included, count as 0)."""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7fffffff), ia), np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


@pytest.mark.parametrize('name', list(MR.GPU_CASES))
def test_kernel_matches_the_restatement(name, _margins):
    case = MR.build_case(name)
    ref = case['ref']
    t = run(case)
    joints, conf, report = t.joints.cpu().numpy(), t.conf.cpu().numpy(), t.report.cpu().numpy()
    bits = t.inliers.cpu().numpy().astype(np.int64)
    # the discrete outputs and the NaN pattern are equal
    assert np.array_equal(report[..., 0], ref['report'][..., 0]) and np.array_equal(report[..., 3], ref['report'][..., 3])
    assert np.array_equal(bits, ref['inliers'].astype(np.int64))
    assert np.array_equal(np.isnan(joints), np.isnan(ref['joints'])) and np.array_equal(np.isnan(report), np.isnan(ref['report']))
    has = ref['report'][..., 0] > 0
    assert np.array_equal(np.isnan(joints).any(-1), ~has) and (conf[~has] == 0).all() and (bits[~has] == 0).all()
    if has.any():
        scale = np.maximum(1.0, np.linalg.norm(ref['joints'][has], axis=-1))
        dj = (np.abs(joints[has] - ref['joints'][has]).max(-1) / scale).max()
        drms = (np.abs(report[has][:, 1] - ref['report'][has][:, 1]) / ref['report'][has][:, 1]).max()
        dsig = (np.abs(report[has][:, 2] - ref['report'][has][:, 2]) / ref['report'][has][:, 2]).max()
        dconf = ulps32(conf, ref['conf']).max()
        print(f'{name}: joints {dj:.3e} m (relative to max(1, |X|)), rms {drms:.3e}, sigma_m {dsig:.3e} relative, conf {dconf} ulp; '
              f'{int(has.sum())} of {has.size} points have a result')
        record('gpu', 'joints_m', dj)
        record('gpu', 'rms_rel', drms)
        record('gpu', 'sigma_rel', dsig)
        record('gpu', 'conf_ulp', dconf)
        assert dj <= BAR and drms <= BAR and dsig <= BAR and dconf <= 1
    if case['want_undistorted']:
        und, want = t.keypoints_und.cpu().numpy(), ref['keypoints_und']
        d = ulps32(und, want)
        record('gpu', 'keypoints_und_ulp', d.max())
        assert d.max() <= 1
        seen = MR.observed(case['keypoints'].astype(np.float64), 0.2)
        assert np.array_equal(und[~seen].view(np.uint32), case['keypoints'][~seen].view(np.uint32))          # passes through as given
        assert np.array_equal(und[..., 2].view(np.uint32), case['keypoints'][..., 2].view(np.uint32))
    else:
        assert t.keypoints_und is None


def test_options_move_kernel_and_restatement_alike(_margins):
    """min_views, refine, tau_px, conf_min and min_angle_deg reach the kernel: the salted five-view case under other options."""
    case = MR.build_case('five_views_salted')
    for kw in (dict(min_views=3), dict(refine=0), dict(refine=1, tau_px=6.0), dict(conf_min=0.6, min_angle_deg=20.0)):
        rkw = {('min_angle_rad' if k == 'min_angle_deg' else k): (np.deg2rad(v) if k == 'min_angle_deg' else v) for k, v in kw.items()}
        ref = MR.triangulate(case['keypoints'], case['cams'], rigid=case['rigid'], **rkw)
        assert len(MR.margins_ok(ref)) == 0
        t = run(case, **kw)
        report, joints = t.report.cpu().numpy(), t.joints.cpu().numpy()
        assert np.array_equal(report[..., 0], ref['report'][..., 0]) and np.array_equal(report[..., 3], ref['report'][..., 3])
        assert np.array_equal(t.inliers.cpu().numpy().astype(np.int64), ref['inliers'].astype(np.int64))
        has = ref['report'][..., 0] > 0
        assert has.any() and np.array_equal(np.isnan(joints).any(-1), ~has)
        assert (np.abs(joints[has] - ref['joints'][has]).max(-1) / np.maximum(1.0, np.linalg.norm(ref['joints'][has], axis=-1))).max() <= BAR
        assert (np.abs(report[has][:, 1:3] - ref['report'][has][:, 1:3]) / ref['report'][has][:, 1:3]).max() <= BAR


def test_the_contract_case_matches_the_restatement():
    """The inputs of `multiview[...]` (tests/header_cases.py), which the four contract families only compare with themselves bit for
    bit, held to the restatement with this module's bars."""
    import header_cases as HC
    i = HC.multiview_inputs(7)
    out = dict(HC.multiview_call(HC.tensors(HC.multiview_inputs, 7, lambda t: t.to(DEV))))
    ref = MR.triangulate(i['kp'], i['cams'], rigid=i['rigid'])
    assert len(MR.margins_ok(ref)) == 0
    assert np.array_equal(out['inliers'].cpu().numpy().astype(np.int64), ref['inliers'].astype(np.int64))
    has = ref['report'][..., 0] > 0
    d = np.abs(out['joints'].cpu().numpy()[has] - ref['joints'][has]).max(-1) / np.maximum(1.0, np.linalg.norm(ref['joints'][has], axis=-1))
    assert has.any() and (~has).any() and d.max() <= BAR


def test_the_same_bits_twice():
    case = MR.build_case('many_points')
    a, b = run(case), run(case)
    for k in ('joints', 'conf', 'report', 'inliers', 'keypoints_und'):
        x, y = getattr(a, k).cpu().numpy(), getattr(b, k).cpu().numpy()
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), k


@pytest.mark.parametrize('name', ['five_views_salted', 'six_views', 'many_points'])
def test_both_group_widths_give_the_same_bits(name):
    """Up to six views a point has 16 lanes, above a wave.  Two more views that observe nothing (confidence 0) take the same points
    through the wave-wide form: the pairs keep their order, the sums their terms, so every output keeps its bits."""
    from rohm_amd.multiview import triangulate
    case = MR.build_case(name)
    kp, cams = case['keypoints'], case['cams']
    V = kp.shape[0]
    assert V <= 6
    blind = kp[:2].copy()
    blind[..., 2] = 0.0
    a = triangulate(_dev(kp), _dev(cams), want_undistorted=True)
    b = triangulate(_dev(np.concatenate([kp, blind])), _dev(np.concatenate([cams, cams[:2]])), want_undistorted=True)
    torch.cuda.synchronize()
    for k in ('joints', 'conf', 'report', 'inliers'):
        x, y = getattr(a, k).cpu().numpy(), getattr(b, k).cpu().numpy()
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), k
    assert torch.equal(a.keypoints_und.view(torch.int32), b.keypoints_und[:V].view(torch.int32))
    assert torch.equal(b.keypoints_und[V:].view(torch.int32), _dev(blind).view(torch.int32))


@pytest.mark.parametrize('name', ['five_views_salted', 'sixteen_views', 'many_points'])
def test_view_residuals_match_the_restatement(name):
    from rohm_amd.multiview import triangulate, view_residuals
    case = MR.build_case(name)
    kp, cams = _dev(case['keypoints']), _dev(case['cams'])
    # of the restatement's joints: the same input on both sides
    got = view_residuals(_dev(case['world']), kp, cams).cpu().numpy()
    want = case['ref_resid']
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isfinite(want).any() and np.isnan(want).any()
    ok = np.isfinite(want)
    d = (np.abs(got[ok] - want[ok]) / want[ok]).max()
    record('gpu', 'resid_rel', d)
    assert d <= BAR
    # of the kernel's own result: the joints differ by at most BAR metres, which moves a projection by f / z BAR = 3e-7 px at most
    own = triangulate(kp, cams).joints
    got_own = view_residuals(own, kp, cams).cpu().numpy()
    assert np.array_equal(np.isnan(got_own), np.isnan(want))
    assert np.abs(got_own[ok] - want[ok]).max() <= 1e-6


def test_noise_free_distorted_keypoints_leave_no_residual():
    from rohm_amd.multiview import pack_cameras, triangulate, view_residuals
    cams = pack_cameras(*MR.make_rig(4, 201, True))
    kp, X = MR.make_views(cams, 3, 25, 202, noise_px=0.0)
    t = triangulate(_dev(kp), _dev(cams))
    resid = view_residuals(t.joints, _dev(kp), _dev(cams)).cpu().numpy()
    err = np.linalg.norm(t.joints.cpu().numpy() - X, axis=-1).max()
    print(f'noise-free, distorted: largest residual {resid.max():.3e} px (bar {RESIDUAL_BAR_PX:.3e}), largest error {err:.3e} m')
    record('gpu', 'noise_free_residual_px', resid.max())
    assert np.isfinite(resid).all() and resid.max() <= RESIDUAL_BAR_PX
    assert (t.report[..., 0] == 4).all() and err <= 1e-6                    # float32 pixels at 4 m and f = 1000: 6e-5 px are 2.4e-7 m


def test_wrappers_refuse_bad_arguments():
    from rohm_amd._lib import RohmHipError
    from rohm_amd.multiview import triangulate, view_residuals
    case = MR.build_case('three_views')
    kp, cams = _dev(case['keypoints']), _dev(case['cams'])
    with pytest.raises(ValueError, match='cams must be'):
        triangulate(kp, cams[:2])
    with pytest.raises(ValueError, match='keypoints must be'):
        triangulate(kp[..., :2], cams)
    with pytest.raises(ValueError, match='rigid must be'):
        triangulate(kp, cams, rigid=torch.zeros(7, device=DEV, dtype=torch.float64))
    with pytest.raises(RohmHipError, match='min_views'):
        triangulate(kp, cams, min_views=4)
    with pytest.raises(RohmHipError, match='tau_px'):
        triangulate(kp, cams, tau_px=-1.0)
    with pytest.raises(ValueError, match='joints_world must be'):
        view_residuals(torch.zeros(2, 22, 3, device=DEV, dtype=torch.float64), kp, cams)
    empty = triangulate(kp[:, :0], cams, want_undistorted=True)             # N == 0: no launch, empty outputs
    assert empty.joints.shape == (0, 22, 3) and empty.keypoints_und.shape == (3, 0, 22, 3)
    rg = _dev(case['rigid'])
    a = triangulate(kp, cams, rigid=rg)
    b = triangulate(kp, cams, rigid=torch.cat([rg[:9].reshape(3, 3), rg[9:].reshape(3, 1)], 1))
    assert torch.equal(a.joints, b.joints)                                   # [3,4] R|t is the same rigid motion


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
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


def test_cli_from_four_views_to_a_track(tmp_path, body_dir, capsys):
    """N = 12 frames of a walking synthetic body seen by four distorting cameras, noise-free -> `python -m rohm_amd.multiview` -> a
    skeleton -> `python -m rohm_amd.fit` -> a track that `read_track` accepts (world_up_axis was given) and whose joints are within
    2 mm of the clean ones.  View 2 has a left / right swap of the wrists in every frame, which must be rejected, not averaged in."""
    from rohm_amd import fit, multiview
    from rohm_amd.data_loaders.track import TRACK_KEYS, read_track
    from rohm_amd.floor import track_joints
    N = 12
    clean = FR.make_frames(synth.synthetic_smplx_tensors(0), N, seed=61, pose_scale=0.12, walk=True, root_angle=0.5, centre=(0.0, 0.0, 1.0))[0].astype(np.float64)
    K, W, D = MR.make_rig(4, 62, True)
    cams = multiview.pack_cameras(K, W, D)
    px, depth = MR.project(cams, clean.reshape(-1, 3))
    assert (depth > 1.0).all()
    kp = np.concatenate([px, np.ones(px.shape[:2] + (1,))], -1).reshape(4, N, 22, 3).astype(np.float32)
    kp[2, :, [20, 21]] = kp[2, :, [21, 20]]
    views, skel, js = str(tmp_path / 'views.npz'), str(tmp_path / 'skeleton.npz'), str(tmp_path / 'report.json')
    np.savez(views, keypoints_2d=kp, camera_mtx=K, world2cam=W, dist_coeffs=D, fps=30.0, world_up_axis=np.array('z'), recording_name=np.array('rig'))
    assert multiview.main(['--views', views, '--out', skel, '--ref_view', '1', '--json', js, '--device', DEV]) == 0
    text = capsys.readouterr().out
    assert 'points triangulated / without result:  %d / 0 of %d' % (N * 22, N * 22) in text and 'median sigma_m' in text and 'wrote' in text
    with open(js) as f:
        rep = json.load(f)
    s = rep['summary']
    assert s['inlier_histogram'] == {'3': 2 * N, '4': 20 * N} and len(rep['report']) == N * 22 and rep['options']['ref_view'] == 1
    assert [r['rejected_share'] for r in s['per_view']] == [0.0, 0.0, pytest.approx(2 / 22), 0.0]
    assert s['per_view'][2]['residual_p95_px'] > 10.0 > s['per_view'][0]['residual_p95_px']
    with np.load(skel, allow_pickle=False) as f:
        skeleton = {k: f[k] for k in f.files}
    assert set(skeleton) <= set(fit.SKELETON_KEYS) | set(fit.PASS_THROUGH)
    in_ref = clean @ W[1, :3, :3].T + W[1, :3, 3]
    d_tri = np.linalg.norm(skeleton['joints_3d'].astype(np.float64) - in_ref, axis=-1).max()
    out = str(tmp_path / 'track.npz')
    assert fit.main(['--skeleton', skel, '--out', out, '--body_model_path', body_dir, '--device', DEV]) == 0
    capsys.readouterr()
    with np.load(out, allow_pickle=False) as f:
        track = {k: f[k] for k in f.files}
    assert set(track) <= set(TRACK_KEYS) and {'cam2world', 'up_axis', 'keypoints_2d', 'focal_length', 'camera_center'} <= set(track)
    rec = read_track(out)
    assert rec['valid'].all()
    _, _, fitted = track_joints(out, body_dir, DEV)
    d_fit = np.linalg.norm(fitted.cpu().numpy().astype(np.float64) - in_ref, axis=-1).max()
    print(f'end to end: triangulated joints {d_tri:.3e} m, fitted joints {d_fit:.3e} m from the clean ones (bar 2e-3)')
    record('gpu', 'end_to_end_triangulated_m', d_tri)
    record('gpu', 'end_to_end_fitted_m', d_fit)
    assert d_tri <= 2e-3 and d_fit <= 2e-3
