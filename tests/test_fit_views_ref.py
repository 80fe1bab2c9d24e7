"""CPU: the float64 restatement of `rohm_fit_views_pose` (tests/fit_views_ref.py) held to what does not depend on it -- central
finite differences, the explicitly stacked Jacobian, a planted translation, multiview_ref's undistortion, a symmetry of the pinhole
camera and planted bodies -- plus the statuses and the argument checks of the entry point (they come before any launch).
tests/test_gpu_fit_views.py then holds the kernel to the restatement."""

import numpy as np
import pytest
import torch

import fit_ref as FR
import fit_views_ref as VR
import multiview_ref as MR
from rohm_amd import fit_views
from rohm_amd.utils import synth

NJ, NX, NROT = VR.NJ, VR.NX, VR.NROT
CACHE = {}


def tensors():
    if 'tensors' not in CACHE:
        CACHE['tensors'] = synth.synthetic_smplx_tensors(0)
        CACHE['mdl'] = FR.model(CACHE['tensors'])
    return CACHE['tensors']


def mdl():
    tensors()
    return CACHE['mdl']


def frame(V, seed, sigma_px=0.0, noise_px=2.0, distorted=(0,)):
    """One frame's worth of the restatement's inputs at a point 0.05 rad off the planted pose."""
    cams = VR.make_rig(V, seed, distorted=distorted)
    joints, truth, betas = VR.make_body(tensors(), 1, seed + 1, beta_scale=0.5)
    kp = VR.pepper(VR.make_keypoints(cams, joints, seed + 2, noise_px=noise_px, conf=(0.3, 1.0)), seed + 3)
    a, b, c = VR.observations(kp[:, 0], cams, 0.2)
    g = np.random.Generator(np.random.PCG64(seed + 4))
    x = truth[0] + np.concatenate([g.standard_normal(NROT) * 0.05, g.standard_normal(3) * 0.02])
    w_prior = fit_views.default_w_prior(V)
    mean = np.concatenate([np.zeros(3), x[3:] + g.standard_normal(NX - 3) * 0.02])
    wsm = np.concatenate([np.zeros(3), np.full(NROT - 3, 700.0), np.full(3, 900.0)])
    return dict(rest=FR.rest_joints(mdl(), betas), cams=cams, a=a, b=b, c=c, w_prior=w_prior, mean=mean, wsm=wsm, sigma_px=sigma_px), x, truth[0], kp, betas


@pytest.mark.parametrize('V,sigma_px', ((1, 0.0), (3, 0.0), (3, 4.0)))
def test_gradient_against_central_differences(V, sigma_px):
    """g is the gradient of E / 2.  Central differences with h = 1e-6 on an energy of some 1e3 px^2 whose third derivatives are of
    the order of E itself: truncation 1e-12 E, rounding 1e-16 E / h = 1e-10 E; the bar is 1e-6 of the largest |g|."""
    kw, x, _, _, _ = frame(V, 11 + V, sigma_px)
    H, g, E = VR.normal_equations(mdl(), x, **kw)
    assert np.isfinite(E) and int((kw['c'] > 0).sum()) >= 15 * V
    h, fd = 1e-6, np.zeros(NX)
    for i in range(NX):
        d = np.zeros(NX)
        d[i] = h
        fd[i] = (VR.energy(mdl(), x + d, **kw) - VR.energy(mdl(), x - d, **kw)) / (4.0 * h)
    rel = np.abs(fd - g).max() / np.abs(g).max()
    print(f'V={V} sigma={sigma_px}: |fd - g| / max|g| = {rel:.3e}')
    assert rel <= 1e-6


@pytest.mark.parametrize('sigma_px', (0.0, 4.0))
def test_normal_matrix_against_the_stacked_jacobian(sigma_px):
    kw, x, _, _, _ = frame(3, 21, sigma_px)
    H, g, _ = VR.normal_equations(mdl(), x, **kw)
    Js, r, w = VR.stacked(mdl(), x, kw['rest'], kw['cams'], kw['a'], kw['b'], kw['c'], sigma_px)
    assert Js.shape == (2 * 3 * NJ, NX)
    wp = np.concatenate([np.repeat(kw['w_prior'], 3), np.zeros(3)])
    Hs = Js.T @ (w[:, None] * Js) + np.diag(wp + kw['wsm'])
    gs = Js.T @ (w * r) + wp * x + kw['wsm'] * (x - kw['mean'])
    assert np.abs(H - Hs).max() <= 1e-12 * np.abs(Hs).max() and np.abs(g - gs).max() <= 1e-12 * np.abs(gs).max()
    assert np.array_equal(H, H.T) or np.abs(H - H.T).max() <= 1e-12 * np.abs(H).max()
    if sigma_px > 0:                                                       # the robust weights are below the plain ones, never above
        assert (w <= np.repeat(kw['c'].reshape(-1), 2) + 1e-15).all() and (w[w > 0] < np.repeat(kw['c'].reshape(-1), 2)[w > 0]).any()


@pytest.mark.parametrize('V', (1, 3))
def test_closed_form_translation_recovers_a_planted_one(V):
    """Noise-free views without distortion (so the five undistortion iterations are exact), float64 keypoints kept as given."""
    cams = VR.make_rig(V, 31 + V, distorted=())
    joints, truth, betas = VR.make_body(tensors(), 1, 32 + V)
    px, _ = MR.project(cams, joints[0])
    a, b = MR.undistort(cams, px[..., 0], px[..., 1])
    c = np.full((V, NJ), 0.7)
    # the planted joints are synth's float32 FK of the parameters; take the restatement's own float64 joints so that 'exactly' is float64's
    rest = FR.rest_joints(mdl(), betas)
    P = FR.fk(mdl(), truth[0, :NROT].reshape(NJ, 3), rest)[1] + truth[0, NROT:]
    px, _ = MR.project(cams, P)
    a, b = MR.undistort(cams, px[..., 0], px[..., 1])
    t = VR.start_translation(mdl(), np.concatenate([truth[0, :NROT], np.zeros(3)]), rest, cams, a, b, c)
    print(f'V={V}: |t - planted| = {np.abs(t - truth[0, NROT:]).max():.3e}')
    assert np.abs(t - truth[0, NROT:]).max() <= 1e-9
    # one observation cannot fix a translation: singular
    c1 = np.zeros((V, NJ))
    c1[0, 5] = 1.0
    assert VR.start_translation(mdl(), np.concatenate([truth[0, :NROT], np.zeros(3)]), rest, cams, a, b, c1) is None


def test_undistortion_is_multiview_refs():
    cams = VR.make_rig(3, 41, distorted=(0, 2))
    joints, _, _ = VR.make_body(tensors(), 2, 42)
    kp = VR.pepper(VR.make_keypoints(cams, joints, 43), 44)
    for i in range(2):
        a, b, c = VR.observations(kp[:, i], cams, 0.2)
        k64 = kp[:, i].astype(np.float64)
        with np.errstate(all='ignore'):
            S = MR.observed(k64, 0.2)
            aw, bw = MR.undistort(cams, k64[..., 0], k64[..., 1])
        assert S.any() and (~S).any()
        assert np.array_equal(a[S], aw[S]) and np.array_equal(b[S], bw[S]) and np.array_equal(c > 0, S) and not a[~S].any()
    # ... and it inverts the forward model on a distorted view
    px, _ = MR.project(cams, joints[0])
    a, b = MR.undistort(cams, px[..., 0], px[..., 1])
    back = np.stack(MR.distort(cams, a, b), -1)
    assert np.abs(back - px).max() <= 1e-6


def test_rotation_about_the_optical_axis_keeps_the_energy():
    """One pinhole view with fx = fy and no distortion, sigma_px = 0: turning the body AND its detections about the optical axis by
    the same angle leaves every |r_vj| as it was; the root has no prior, so E is unchanged -- up to the body model's Rodrigues
    convention (angle = |r + 1e-8|), which makes the turned root's axis-angle stand for a rotation some 2e-8 rad off: a joint 1 m
    from the root moves 2e-8 m = 6e-6 px at f / z = 286, and E = sum c r^2 with 22 residuals of up to 10 px moves by up to
    2 * 22 * 10 * 6e-6 = 3e-3 px^2, 1e-6 of E = 3e3 px^2.  The bar is 1e-5 E; a broken symmetry would show at the order of E."""
    cams = VR.make_rig(1, 51, distorted=())
    cams[0, 13] = cams[0, 12]
    joints, truth, betas = VR.make_body(tensors(), 1, 52, root_base=VR.facing(cams))
    kp = VR.make_keypoints(cams, joints, 53)
    rest = FR.rest_joints(mdl(), betas)
    a, b, c = VR.observations(kp[:, 0], cams, 0.2)
    g = np.random.Generator(np.random.PCG64(54))
    x = truth[0] + np.concatenate([g.standard_normal(NROT) * 0.05, g.standard_normal(3) * 0.02])
    w_prior, zeros = fit_views.default_w_prior(1), np.zeros(NX)
    E = VR.energy(mdl(), x, rest, cams, a, b, c, w_prior, zeros, zeros, 0.0)
    R, t = cams[0, :9].reshape(3, 3), cams[0, 9:12]
    phi = 0.7
    Z = np.array([[np.cos(phi), -np.sin(phi), 0.0], [np.sin(phi), np.cos(phi), 0.0], [0.0, 0.0, 1.0]])
    Q = R.T @ Z @ R                                                        # the turn in the world: X -> Q X + q keeps R X + t on the axis' orbit
    q = R.T @ (Z @ t - t)
    x2 = x.copy()
    x2[:3] = FR.log_map(Q @ FR.rodrigues(x[:3]))
    x2[NROT:] = Q @ (rest[0] + x[NROT:]) + q - rest[0]                     # joints are rest-rooted: p_0 = rest_0 whatever the root rotation
    a2, b2 = Z[0, 0] * a + Z[0, 1] * b, Z[1, 0] * a + Z[1, 1] * b
    E2 = VR.energy(mdl(), x2, rest, cams, a2, b2, c, w_prior, zeros, zeros, 0.0)
    print(f'E = {E:.9e}, turned {E2:.9e}')
    assert abs(E2 - E) <= 1e-5 * E


def test_statuses_on_planted_frames():
    cams = VR.make_rig(2, 61, distorted=(0,))
    joints, truth, betas = VR.make_body(tensors(), 5, 62)
    kp = VR.make_keypoints(cams, joints, 63)
    kp[:, 0, 5:, 2] = 0.1                                                  # frame 0: 10 observations, below min_obs = 12
    init = truth.copy()
    init[1, 7] = np.nan                                                    # frame 1: a rotation that is not finite
    init[2, NROT] = np.nan                                                 # frame 2: a translation that is neither three NaN nor finite
    init[3, NROT:] += 2.0 * ((-cams[0, :9].reshape(3, 3).T @ cams[0, 9:12]) - VR.TARGET)      # frame 3: behind camera 0, through its centre
    init[4, NROT:] = np.nan                                                # frame 4: the kernel solves the translation
    b = np.repeat(betas[None].astype(np.float32), 5, axis=0)
    p, r, s, n = VR.fit_views_pose(mdl(), kp, cams, b, init, w_prior=fit_views.default_w_prior(2), iters=3, want_normal=True)
    assert r[:, 0].tolist() == [0, 2, 2, 3, 1] and r[:, 6].tolist() == [10, 44, 44, 44, 44]
    bad = r[:, 0] != 1
    assert not p[bad].any() and not n[bad].any() and np.isnan(s[:, bad]).all() and np.isnan(r[bad][:, [1, 2, 4, 5, 7]]).all() and not r[bad, 3].any()
    assert r[4, 2] < r[4, 1] and r[4, 7] > 1.0 and np.isfinite(s[:, 4]).all() and np.abs(p[4, NROT:] - truth[4, NROT:]).max() < 0.05
    # a singular translation system is status 3 as well: one observation gives two equations for three unknowns
    kp2 = kp.copy()
    kp2[:, 4, :, 2] = 0.0
    kp2[0, 4, 9, 2] = 1.0
    r2 = VR.fit_views_pose(mdl(), kp2, cams, b, init, w_prior=fit_views.default_w_prior(2), iters=0, min_obs=1)[1]
    assert r2[4, 0] == 3 and r2[4, 6] == 1


def test_start_rows_face_the_camera_and_turn_the_back():
    cams = VR.make_rig(3, 71)
    rows = fit_views.start_rows(cams, 1)
    assert rows.shape == (2, NX) and np.isnan(rows[:, NROT:]).all() and not rows[:, 3:NROT].any()
    R = cams[1, :9].reshape(3, 3)
    for row, fwd in ((rows[0], -1.0), (rows[1], 1.0)):
        B = R @ FR.rodrigues(row[:3])                                      # body axes in the camera: y (up) is the image's up, z (forward) to or from it
        assert np.allclose(B[:, 1], [0.0, -1.0, 0.0], atol=1e-7) and np.allclose(B[:, 2], [0.0, 0.0, fwd], atol=1e-7)
    with pytest.raises(ValueError, match='ref_view'):
        fit_views.start_rows(cams, 3)


def test_the_kernel_refuses_cpu_tensors():
    kp, cams = torch.zeros(1, 1, 22, 3), torch.zeros(1, 24, dtype=torch.float64)
    with pytest.raises(Exception, match='no CPU fallback'):
        fit_views.fit_views_pose(None, kp, cams, torch.zeros(1, 10), torch.zeros(1, 69, dtype=torch.float64))


def test_argument_errors_name_the_argument():
    """The checks come before any launch and touch no pointer, so they run without a GPU."""
    from rohm_amd import _lib
    L = _lib.lib()

    def call(V=2, N=1, iters=1, min_obs=12, sigma=0.0, conf_min=0.2, ws=0.0, wst=0.0, h=8, kp=8, cams=8, betas=8, init=8, wp=8, params=8, report=8):
        return L.rohm_fit_views_pose(h, kp, cams, betas, init, None, wp, ws, wst, sigma, conf_min, iters, min_obs, V, N, params, report, None, None, None)
    nan, inf = float('nan'), float('inf')
    for kw, word in ((dict(V=0), 'V must be'), (dict(V=17), 'V must be'), (dict(N=-1), 'N must be'), (dict(iters=-1), 'iters'),
                     (dict(sigma=-1.0), 'sigma_px'), (dict(sigma=nan), 'sigma_px'), (dict(conf_min=-0.1), 'conf_min'), (dict(conf_min=inf), 'conf_min'),
                     (dict(ws=-1.0), 'w_smooth '), (dict(ws=nan), 'w_smooth '), (dict(wst=-1.0), 'w_smooth_t'), (dict(wst=inf), 'w_smooth_t'),
                     (dict(min_obs=0), 'min_obs'), (dict(h=None), 'body model'), (dict(kp=None), 'keypoints'), (dict(cams=None), 'cams'),
                     (dict(betas=None), 'betas'), (dict(init=None), 'init'), (dict(wp=None), 'w_prior'), (dict(params=None), 'params'),
                     (dict(report=None), 'report')):
        assert call(**kw) == -1, kw
        assert word in L.rohm_last_error().decode(), (kw, L.rohm_last_error())
    assert call(N=0, h=None, kp=None, cams=None, betas=None, init=None, wp=None, params=None, report=None) == 0


# ---- recovery ----------------------------------------------------------------------------------------------------------------------
# Measured with this restatement on the cases below (4 frames each, pose scale 0.3 rad, cameras 3.5 m away, f = 1000 px, the module's
# default weights, 30 iterations, one smoothing pass) and recorded in profiles/fit_views_parity.json ['recovery']; the bars are those
# values with a factor of 2 for the draw.  (V, pixel noise): (mean joint error, worst joint error) in metres.
MEASURED = {(2, 2.0): (7.33e-3, 19.59e-3), (4, 2.0): (4.20e-3, 12.93e-3), (1, 0.0): (26.94e-3, 45.10e-3)}
RMS_ONE_VIEW = 0.531                 # px, measured likewise: what the prior and the smoothing cost in pixels on noise-free input


@pytest.mark.parametrize('V,noise_px', list(MEASURED))
def test_recovery_of_planted_bodies(V, noise_px):
    N = 4
    cams = VR.make_rig(V, 81 + V, distorted=(0,))
    joints, truth, betas = VR.make_body(tensors(), N, 82 + V, root_base=VR.facing(cams), root_angle=0.5, walk=True)
    kp = VR.make_keypoints(cams, joints, 83 + V, noise_px=noise_px)
    p, r, s, back = VR.fit_views(mdl(), kp, cams, betas, fit_views.start_rows(cams, 0), fit_views.default_w_prior(V), fit_views.W_SMOOTH,
                                 fit_views.W_SMOOTH_T, fit_views.SIGMA_PX)
    assert (r[:, 0] == 1).all()
    err = np.linalg.norm(VR.joints_of(mdl(), p, np.repeat(betas[None], N, axis=0)) - joints, axis=-1)
    print(f'V={V}, {noise_px} px of noise: joint error mean {err.mean() * 1e3:.2f} mm, worst {err.max() * 1e3:.2f} mm; reprojection rms '
          f'{r[:, 5].max():.3f} px; back turned {back.tolist()}')
    VR.record('recovery', f'V{V}_mean_m', err.mean())
    VR.record('recovery', f'V{V}_worst_m', err.max())
    VR.record('recovery', f'V{V}_rms_px', r[:, 5].max())
    mean_bar, worst_bar = (2.0 * m for m in MEASURED[V, noise_px])
    assert err.mean() <= mean_bar and err.max() <= worst_bar
    if V == 1:                                                             # one view: the pixels are met even where the depth is not
        assert r[:, 5].max() <= 2.0 * RMS_ONE_VIEW
