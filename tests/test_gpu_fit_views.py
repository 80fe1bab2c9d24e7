"""GPU: SMPL-X from 2-D keypoints -- `rohm_fit_views_pose` (csrc/fit_views.hip) against its float64 restatement
(tests/fit_views_ref.py, held to finite differences, the stacked Jacobian and planted bodies in tests/test_fit_views_ref.py),
`fit_views` with one view, and `python -m rohm_amd.fit_views` end to end with the synthetic body layer.

Cases (V, N), each with fractional confidences, NaN detections and view 0 distorted: (1, 1); (2, 3), smoothing at both ends and
an unusable middle frame; (3, 70) with 10 iterations, more than a wave of frames; (16, 2), the view limit and the LDS budget.
Every frame starts 0.05 rad off its planted rotations with a NaN translation, so the kernel solves its start translation.

Bars.  (a) H, g, E and the solved start translation: kernel and restatement are both float64 on the same float32 inputs; they
differ by the order of sums of at most 2 * 16 * 22 terms and by the device's sin / cos against the host's, a few ulp: about 1e-13
of the largest magnitude.  The bar is 1e-9 of each frame's largest |H|, of its largest |g|, of E: the bar of test_gpu_fit.py, with
the same derivation.  (b) a near-tie in one accept / reject decision may take kernel and restatement down different, equally good
paths, so the bars on the final energies, `resid` and the fitted joints cannot be derived: they are ten times what was measured
on an MI355X (profiles/fit_views_parity.json: 'full_fit_energy_rel', 'full_fit_resid_px', 'full_fit_joint_m').  Two conditions hold
whatever was measured: E_end <= E_start on every frame, and E_end(kernel) <= 1.05 E_end(restatement) on every frame."""
import json

import numpy as np
import pytest
import torch

import fit_ref as FR
import fit_views_ref as VR
import multiview_ref as MR
import stale_memory as SM
from rohm_amd.utils import synth

record = VR.record
pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NJ, NX, NROT = VR.NJ, VR.NX, VR.NROT
BAR = 1e-9
# ten times the largest values measured on an MI355X over the cases of test_full_fits (profiles/fit_views_parity.json)
ENERGY_BAR = 10 * 7.424e-14            # measured at (1, 1): 7.424e-14 ((2, 3): 5.6e-16, (3, 70): 1.3e-14, (16, 2): 1.6e-15)
RESID_BAR = 10 * 1.600e-07             # px; measured at (3, 70): 1.600e-07 ((1, 1): 3.1e-13, (2, 3): 2.8e-13, (16, 2): 2.1e-10)
JOINT_BAR = 10 * 1.365e-09             # m; measured at (3, 70): 1.365e-09 ((1, 1): 4.7e-14, (2, 3): 8.9e-16, (16, 2): 9.9e-13)
W_SMOOTH, W_SMOOTH_T = 700.0, 900.0

CACHE = {}


def tensors():
    if 'tensors' not in CACHE:
        CACHE['tensors'] = synth.synthetic_smplx_tensors(0)
        CACHE['mdl'] = FR.model(CACHE['tensors'])
    return CACHE['tensors']


def mdl():
    tensors()
    return CACHE['mdl']


def _layer():
    from rohm_amd.body_model import SMPLXLayer
    if 'layer' not in CACHE:
        CACHE['layer'] = SMPLXLayer.from_tensors(tensors()).to(DEV)
    return CACHE['layer']


def nat():
    from rohm_amd.body_model import native_for
    return native_for(_layer(), torch.device(DEV))


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)            # a copy: the shared inputs are read-only


def options(V, N, iters):
    """What a case runs with: robust at 3 views and plain elsewhere, smoothing (towards the planted poses, 0.01 off) at N = 3."""
    from rohm_amd.fit_views import default_w_prior
    case = VR.build_case(tensors(), V, N)
    kw = dict(w_prior=default_w_prior(V), sigma_px=30.0 if V in (2, 3) else 0.0, iters=iters)
    if N == 3:
        kw.update(prev=case['truth'] + 0.01, w_smooth=W_SMOOTH, w_smooth_t=W_SMOOTH_T)
    return case, kw


def run(case, kw, want_normal=False):
    from rohm_amd.fit_views import fit_views_pose
    kw = {k: (_dev(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    out = fit_views_pose(nat(), _dev(case['kp']), _dev(case['cams']), _dev(case['betas']), _dev(case['init']), want_normal=want_normal, **kw)
    return tuple(None if o is None else o.cpu().numpy() for o in out)


def reference(V, N, iters, want_normal=False):
    key = ('ref', V, N, iters, want_normal)
    if key not in CACHE:
        case, kw = options(V, N, iters)
        CACHE[key] = VR.fit_views_pose(mdl(), case['kp'], case['cams'], case['betas'], case['init'], want_normal=want_normal, **kw)
    return CACHE[key]


def same_nan(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b))


# ---- (a) normal equations and the start point ------------------------------------------------------------------------------------
@pytest.mark.parametrize('V,N', list(VR.GPU_CASES), ids=lambda v: str(v))
def test_normal_equations_match_the_restatement(V, N):
    case, kw = options(V, N, 0)
    p_want, r_want, s_want, n_want = reference(V, N, 0, True)
    p, r, s, n = run(case, kw, want_normal=True)
    assert p.shape == (N, NX) and r.shape == (N, 8) and s.shape == (V, N, NJ) and n.shape == (N, NX, NX + 1)
    assert np.array_equal(r[:, 0], r_want[:, 0]) and np.array_equal(r[:, 6], r_want[:, 6])
    if N >= 3:
        assert r_want[:3, 0].tolist() == [1, 0, 1]
    ok = r_want[:, 0] == 1
    assert ok.any() and not p[~ok].any() and not n[~ok].any() and np.isnan(r[~ok][:, [1, 2, 4, 5, 7]]).all() and not r[~ok, 3].any()
    assert np.isnan(s[:, ~ok]).all() and same_nan(s, s_want) and np.isnan(s_want[:, ok]).any() and np.isfinite(s_want[:, ok]).any()
    worst_h = worst_g = worst_e = 0.0
    for i in np.flatnonzero(ok):
        H, g, Hw, gw = n[i, :, :NX], n[i, :, NX], n_want[i, :, :NX], n_want[i, :, NX]
        assert np.array_equal(H, H.T)
        worst_h = max(worst_h, np.abs(H - Hw).max() / np.abs(Hw).max())
        worst_g = max(worst_g, np.abs(g - gw).max() / np.abs(gw).max())
        worst_e = max(worst_e, abs(r[i, 1] - r_want[i, 1]) / r_want[i, 1])
    start = np.abs(p[ok] - p_want[ok]).max() / np.abs(p_want[ok]).max()
    res = np.nanmax(np.abs(s[:, ok] - s_want[:, ok])) / np.nanmax(s_want[:, ok])
    print(f'V={V} N={N}: H {worst_h:.3e}, g {worst_g:.3e}, E {worst_e:.3e}, start point (translation solved) {start:.3e}, resid {res:.3e} of the '
          f'largest (bar {BAR:.0e}); rotations kept: {np.array_equal(p[ok][:, :NROT], case["init"][ok][:, :NROT])}')
    record('gpu', 'normal_H_rel', worst_h)
    record('gpu', 'normal_g_rel', worst_g)
    record('gpu', 'start_point_rel', start)
    assert worst_h <= BAR and worst_g <= BAR and worst_e <= BAR and start <= BAR and res <= BAR
    assert np.array_equal(p[ok][:, :NROT], case['init'][ok][:, :NROT])
    assert np.array_equal(r[ok, 1], r[ok, 2]) and not r[:, 3].any() and (r[ok, 4] == FR.LAMBDA0).all()
    assert np.abs(r[ok, 5] - r_want[ok, 5]).max() <= BAR * r_want[ok, 5].max() and np.abs(r[ok, 7] - r_want[ok, 7]).max() <= BAR * 10.0
    # the same input, the same bits; and without `normal` and `resid` the rest is unchanged
    p2, r2, s2, n2 = run(case, kw, want_normal=True)
    assert p2.tobytes() == p.tobytes() and r2.tobytes() == r.tobytes() and s2.tobytes() == s.tobytes() and n2.tobytes() == n.tobytes()
    p3, r3, s3, _ = run(case, dict(kw, want_resid=False))
    assert s3 is None and p3.tobytes() == p.tobytes() and r3.tobytes() == r.tobytes()


# ---- (b) full fits -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('V,N', list(VR.GPU_CASES), ids=lambda v: str(v))
def test_full_fits(V, N):
    iters = VR.GPU_CASES[V, N]
    case, kw = options(V, N, iters)
    p_want, r_want, s_want, _ = reference(V, N, iters)
    p, r, s, _ = run(case, kw)
    assert np.array_equal(r[:, 0], r_want[:, 0])
    ok = r_want[:, 0] == 1
    assert not p[~ok].any() and same_nan(s, s_want)
    e_rel = np.abs(r[ok, 2] - r_want[ok, 2]) / r_want[ok, 2]
    s_abs = np.nanmax(np.abs(s[:, ok] - s_want[:, ok]))
    jd = np.linalg.norm(VR.joints_of(mdl(), p[ok], case['betas'][ok]) - VR.joints_of(mdl(), p_want[ok], case['betas'][ok]), axis=-1)
    ratio = r[ok, 2] / r_want[ok, 2]
    err = np.linalg.norm(VR.joints_of(mdl(), p[ok], case['betas'][ok]) - case['joints'][ok], axis=-1)
    print(f'V={V} N={N}, {iters} iterations, {int(ok.sum())} frames fitted: |E_end - restatement| / E_end max {e_rel.max():.3e} (bar {ENERGY_BAR:.3e}), '
          f'resid max {s_abs:.3e} px (bar {RESID_BAR:.3e}), joints of the fitted parameters max {jd.max():.3e} m (bar {JOINT_BAR:.3e}); '
          f'E_end / restatement in [{ratio.min():.6f}, {ratio.max():.6f}]; accepted {r[ok, 3].min():.0f} .. {r[ok, 3].max():.0f}, '
          f'E_end / E_start max {(r[ok, 2] / r[ok, 1]).max():.3e}, rms max {r[ok, 5].max():.2f} px, against the planted joints {err.mean() * 1e3:.1f} mm')
    record('gpu', 'full_fit_energy_rel', e_rel.max())
    record('gpu', 'full_fit_resid_px', s_abs)
    record('gpu', 'full_fit_joint_m', jd.max())
    record('gpu', 'full_fit_energy_ratio_max', ratio.max())
    assert (r[ok, 2] <= r[ok, 1]).all()
    assert (r[ok, 2] <= 1.05 * r_want[ok, 2]).all()
    assert (r[ok, 3] >= 1).all() and (r[ok, 3] <= iters).all() and (r[ok, 7] > 1.0).all()
    assert e_rel.max() <= ENERGY_BAR
    assert s_abs <= RESID_BAR
    assert jd.max() <= JOINT_BAR


# ---- (c) one view's mis-detection --------------------------------------------------------------------------------------------------------
def test_a_planted_outlier_saturates_only_with_the_robust_function():
    """Four views, 1 px of noise, joint 7 (the left ankle) of view 2 moved by 80 px.  Robust (sigma_px = 30): that view's residual at
    the joint stays near 80 px and the other views' stay small; plain: the joint is dragged, the outlier's residual shrinks and the
    others' grow.  The bars are the restatement's own figures on the same input, with 10 % of margin."""
    from rohm_amd.fit_views import default_w_prior, fit_views_pose
    V, N, J, BAD = 4, 2, 7, 2
    cams = VR.make_rig(V, 601, distorted=(0,))
    joints, truth, betas = VR.make_body(tensors(), N, 602, root_base=VR.facing(cams), root_angle=0.6)
    kp = VR.make_keypoints(cams, joints, 603, noise_px=1.0)
    kp[BAD, :, J, 0] += 80.0
    g = np.random.Generator(np.random.PCG64(604))
    init = truth + np.concatenate([g.standard_normal((N, NROT)) * 0.03, np.zeros((N, 3))], axis=1)
    b = np.repeat(betas[None].astype(np.float32), N, axis=0)
    others = [v for v in range(V) if v != BAD]
    got, want = {}, {}
    for sigma in (30.0, 0.0):
        kw = dict(w_prior=default_w_prior(V), sigma_px=sigma, iters=20)
        want[sigma] = VR.fit_views_pose(mdl(), kp, cams, b, init, **kw)[2]
        got[sigma] = fit_views_pose(nat(), _dev(kp), _dev(cams), _dev(b), _dev(init), **dict(kw, w_prior=_dev(kw['w_prior'])))[2].cpu().numpy()
    hi, lo = 0.9 * want[30.0][BAD, :, J].min(), 1.1 * want[30.0][others][:, :, J].max()
    print(f'robust: outlier {got[30.0][BAD, :, J]} px (restatement {want[30.0][BAD, :, J]}), the other views at the joint at most '
          f'{got[30.0][others][:, :, J].max():.2f} px (restatement {want[30.0][others][:, :, J].max():.2f}); plain: outlier {got[0.0][BAD, :, J]} px, '
          f'the others at most {got[0.0][others][:, :, J].max():.2f} px (restatement {want[0.0][others][:, :, J].max():.2f})')
    assert hi > 60.0 and lo < 6.0                                           # the restatement itself: near the planted 80 px, and a few px
    assert (got[30.0][BAD, :, J] >= hi).all() and got[30.0][others][:, :, J].max() <= lo
    assert (got[0.0][BAD, :, J] < hi).all() and (got[0.0][others][:, :, J].max(axis=0) > lo).all()
    assert (want[0.0][BAD, :, J] < hi).all() and (want[0.0][others][:, :, J].max(axis=0) > lo).all()


# ---- (d) one view: the candidate with the smaller energy ------------------------------------------------------------------------------------
def test_fit_views_with_one_view_picks_the_restatements_candidate():
    from rohm_amd import fit_views as FV
    cams = VR.make_rig(1, 611)
    parts = [VR.make_body(tensors(), 1, 612 + i, root_base=VR.facing(cams, back=bool(i % 2)), root_angle=0.3, pose_scale=0.2) for i in range(4)]
    joints = np.concatenate([p[0] for p in parts])
    kp = VR.make_keypoints(cams, joints, 616, noise_px=1.0)
    kw = dict(w_smooth=FV.W_SMOOTH, w_smooth_t=FV.W_SMOOTH_T, sigma_px=FV.SIGMA_PX, iters=12, smooth_passes=1)
    pw, rw, sw, back_want = VR.fit_views(mdl(), kp, cams, np.zeros(10), FV.start_rows(cams, 0), FV.default_w_prior(1), **kw)
    res = FV.fit_views(kp, cams, body_model=_layer(), device=DEV, **kw)
    print(f'back turned: {res.back_turned.tolist()} (restatement {back_want.tolist()}); rms {res.report[:, 5]} px (restatement {rw[:, 5]})')
    assert back_want.tolist() == [False, True, False, True]
    assert res.valid.all() and np.array_equal(res.back_turned, back_want) and not res.warm_started.any()
    assert (res.report[:, 2] <= 1.05 * rw[:, 2]).all() and res.resid.shape == (1, 4, NJ)


# ---- (e) end to end ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def body_dir(tmp_path_factory):
    """SMPLX_NEUTRAL.npz in the released layout from the synthetic model."""
    t = tensors()
    nv = t['v_template'].shape[0]
    kt = np.stack([np.array(synth.SMPLX_PARENTS), np.arange(55)]).astype(np.int64)
    kt[0, 0] = 2 ** 32 - 1
    d = tmp_path_factory.mktemp('body')
    np.savez(str(d / 'SMPLX_NEUTRAL.npz'), v_template=t['v_template'].numpy(), shapedirs=t['shapedirs'].numpy(),
             posedirs=t['posedirs'].numpy().T.reshape(nv, 3, 486), J_regressor=t['J_regressor'].numpy(), kintree_table=kt,
             weights=t['lbs_weights'].numpy(), f=np.zeros((4, 3), np.int64))
    return str(d)


@pytest.mark.parametrize('V', (4, 1))
def test_cli_from_a_body25_views_file_to_a_track(V, tmp_path, body_dir, capsys):
    """N = 6 frames of the walking synthetic body seen by V cameras (2 px of noise with four, none with one) as a BODY_25 views file ->
    `python -m rohm_amd.fit_views --ref_view` -> a track that `read_track` accepts, in the reference camera's frame.  Four views: the
    joints (`floor.track_joints`, float32) against the planted ones at the observed joints; the bar is twice what the restatement
    reaches on the same input (float32 storage, path forks).  One view: the reprojection rms against twice the restatement's -- the
    3-D error of one view is not held to anything."""
    from rohm_amd.data_loaders.dataloader_video import OPENPOSE_TO_SMPL
    from rohm_amd.data_loaders.track import TRACK_KEYS, read_track
    from rohm_amd import fit_views as FV
    from rohm_amd.fit import BODY25_PROXY
    from rohm_amd.floor import track_joints
    N, ref, iters = 6, V - 1, 15
    K, W, D = MR.make_rig(V, 621 + V, True, radius=3.5, target=VR.TARGET)
    cams = FV.multiview.pack_cameras(K, W, D)
    joints, truth, betas = VR.make_body(tensors(), N, 622 + V, root_base=VR.facing(cams, ref), root_angle=0.4, walk=True)
    kp22 = VR.make_keypoints(cams, joints, 623 + V, noise_px=2.0 if V > 1 else 0.0)
    observed = [s for s in range(NJ) if s not in BODY25_PROXY]
    kp25 = np.zeros((V, N, 25, 3), np.float32)
    for s in observed:
        kp25[:, :, OPENPOSE_TO_SMPL[s]] = kp22[:, :, s]
    views, out, js = str(tmp_path / 'views.npz'), str(tmp_path / 'track.npz'), str(tmp_path / 'report.json')
    np.savez(views, keypoints_2d=kp25, camera_mtx=K, world2cam=W, dist_coeffs=D, fps=30.0, world_up_axis=np.array('z'), floor_height=0.0,
             recording_name=np.array('walk'))
    assert FV.main(['--views', views, '--out', out, '--body_model_path', body_dir, '--json', js, '--device', DEV, '--ref_view', str(ref),
                    '--iters', str(iters)]) == 0
    text = capsys.readouterr().out
    assert f'{N} of {N} frames fitted from {V} view' in text and 'wrote' in text and ('one view' in text) == (V == 1)
    with np.load(out, allow_pickle=False) as f:
        track = {k: f[k] for k in f.files}
    assert set(track) <= set(TRACK_KEYS) and set(track) == {'global_orient', 'transl', 'body_pose', 'betas', 'valid', 'fps', 'cam2world', 'up_axis',
                                                            'floor_height', 'recording_name', 'keypoints_2d', 'focal_length', 'camera_center'}
    rec = read_track(out)
    assert rec['valid'].all() and track['keypoints_2d'].shape == (N, 25, 3) and np.allclose(track['cam2world'], np.linalg.inv(W[ref]))
    assert np.array_equal(track['focal_length'], [K[ref, 0, 0], K[ref, 1, 1]])
    with open(js) as f:
        rep = json.load(f)
    assert rep['summary']['fitted'] == N and len(rep['report']) == N and rep['options']['ref_view'] == ref
    # the restatement on the same input: the cameras relative to the reference view, the proxies unobserved
    rel = FV.multiview.pack_cameras(K, W @ np.linalg.inv(W[ref])[None], D)
    kps = kp22.copy()
    kps[:, :, list(BODY25_PROXY), 2] = 0.0
    pw, rw, _, _ = VR.fit_views(mdl(), kps, rel, np.zeros(10), FV.start_rows(rel, ref), FV.default_w_prior(V), FV.W_SMOOTH, FV.W_SMOOTH_T, FV.SIGMA_PX,
                                iters=iters)
    planted = joints @ W[ref, :3, :3].T + W[ref, :3, 3]
    want = np.linalg.norm(VR.joints_of(mdl(), pw, np.zeros((N, 10)))[:, observed] - planted[:, observed], axis=-1)
    _, _, fitted = track_joints(out, body_dir, DEV)
    d = np.linalg.norm(fitted.cpu().numpy().astype(np.float64)[:, observed] - planted[:, observed], axis=-1)
    rms, rms_want = np.array([row[5] for row in rep['report']]), rw[:, 5]
    print(f'end to end, {V} views: joints against the planted ones max {d.max() * 1e3:.2f} mm, mean {d.mean() * 1e3:.2f} mm (restatement {want.max() * 1e3:.2f} / '
          f'{want.mean() * 1e3:.2f} mm); reprojection rms max {rms.max():.3f} px (restatement {rms_want.max():.3f} px)')
    record('end_to_end', f'V{V}_joint_worst_m', d.max())
    record('end_to_end', f'V{V}_joint_worst_m_restatement', want.max())
    record('end_to_end', f'V{V}_rms_px', rms.max())
    record('end_to_end', f'V{V}_rms_px_restatement', rms_want.max())
    if V > 1:
        assert d.max() <= 2.0 * want.max() and d.mean() <= 2.0 * want.mean()
    assert rms.max() <= 2.0 * rms_want.max()


# ---- (f) stale memory ---------------------------------------------------------------------------------------------------------------------
def _all_outputs():
    from rohm_amd.fit_views import fit_views_pose
    out = []
    for (V, N), iters in (((3, 70), 2), ((2, 3), 3)):
        case, kw = options(V, N, iters)
        kw = {k: (_dev(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
        p, r, s, n = fit_views_pose(nat(), _dev(case['kp']), _dev(case['cams']), _dev(case['betas']), _dev(case['init']), want_normal=True, **kw)
        out += [(f'params_{V}', p), (f'report_{V}', r), (f'resid_{V}', s), (f'normal_{V}', n)]
    torch.cuda.synchronize()
    return out


def test_outputs_do_not_depend_on_what_their_memory_held():
    with SM.poison(SM.ZEROS):
        want = _all_outputs()
    for name, word in SM.PATTERNS.items():
        with SM.poison(word):
            got = _all_outputs()
        for (label, a), (_, b) in zip(want, got):
            assert SM.first_difference(a, b) is None, (name, label, SM.first_difference(a, b))


def test_the_contract_case_matches_the_restatement():
    """The inputs of `fit_views[...]` (tests/header_cases.py), which the four contract families only compare with themselves bit for
    bit, held to the restatement: statuses, normal equations and start energy with bar (a), and the two conditions on E_end."""
    import header_cases as HC
    i = HC.fit_views_inputs(7)
    out = dict(HC.fit_views_call(HC.tensors(HC.fit_views_inputs, 7, lambda t: t.to(DEV))))
    ws, wst, sigma, conf_min, iters, min_obs = HC.FV_SCALARS[0]
    pw, rw, sw, nw = VR.fit_views_pose(mdl(), i['kp'], i['cams'], i['betas'], i['init'], prev=i['prev'], w_prior=i['w_prior'], w_smooth=ws,
                                       w_smooth_t=wst, sigma_px=sigma, conf_min=conf_min, iters=iters, min_obs=min_obs, want_normal=True)
    r, n = out['report'].cpu().numpy(), out['normal'].cpu().numpy()
    assert rw[:, 0].tolist() == [1, 0, 1] and np.array_equal(r[:, 0], rw[:, 0]) and np.array_equal(r[:, 6], rw[:, 6])
    for f in (0, 2):
        assert np.abs(n[f] - nw[f]).max() <= BAR * np.abs(nw[f]).max() and abs(r[f, 1] - rw[f, 1]) <= BAR * rw[f, 1]
        assert r[f, 2] <= r[f, 1] and r[f, 2] <= 1.05 * rw[f, 2]


# ---- bad arguments --------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_by_name():
    from rohm_amd import _lib
    from rohm_amd.fit_views import default_w_prior, fit_views_pose
    lib, stream = _lib.lib(), _lib.stream_ptr(torch.device(DEV))
    case, _ = options(2, 3, 1)
    kp, cams, b, init = (_dev(case[k]) for k in ('kp', 'cams', 'betas', 'init'))
    wp = _dev(default_w_prior(2))
    params, report = torch.empty(3, NX, device=DEV, dtype=torch.float64), torch.empty(3, 8, device=DEV, dtype=torch.float64)
    h = nat().handle

    def pose(V=2, N=3, iters=1, min_obs=12, sigma=0.0, conf_min=0.2, ws=0.0, wst=0.0, handle=h, kpp=kp.data_ptr(), initp=init.data_ptr()):
        return lib.rohm_fit_views_pose(handle, kpp, cams.data_ptr(), b.data_ptr(), initp, None, wp.data_ptr(), ws, wst, sigma, conf_min, iters, min_obs,
                                       V, N, params.data_ptr(), report.data_ptr(), None, None, stream)
    assert pose() == 0 and pose(N=0, handle=None, kpp=None) == 0
    for kw, word in ((dict(V=0), b'V must be'), (dict(V=17), b'V must be'), (dict(N=-1), b'N must be'), (dict(iters=-1), b'iters'),
                     (dict(sigma=float('nan')), b'sigma_px'), (dict(conf_min=-1.0), b'conf_min'), (dict(ws=-1.0), b'w_smooth '),
                     (dict(wst=float('inf')), b'w_smooth_t'), (dict(min_obs=0), b'min_obs'), (dict(kpp=None), b'keypoints'), (dict(initp=None), b'init'),
                     (dict(handle=None), b'body model')):
        assert pose(**kw) == -1 and word in lib.rohm_last_error(), kw
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match=r'\[V, N, 22, 3\]'):
        fit_views_pose(nat(), kp[:, :, :21], cams, b, init)
    with pytest.raises(ValueError, match=r'cams must be'):
        fit_views_pose(nat(), kp, cams[:1], b, init)
    with pytest.raises(ValueError, match=r'betas must be'):
        fit_views_pose(nat(), kp, cams, b[:2], init)
    with pytest.raises(ValueError, match=r'init must be'):
        fit_views_pose(nat(), kp, cams, b, None)
    with pytest.raises(ValueError, match=r'prev must be'):
        fit_views_pose(nat(), kp, cams, b, init, prev=init[:, :66])
    with pytest.raises(_lib.RohmHipError):
        fit_views_pose(nat(), kp.cpu(), cams, b, init)
