"""TEST INFRASTRUCTURE ONLY: the cases that hold include/rohm_multiview.h, rohm_fit_views.h and rohm_rig.h to the four contracts of
include/rohm_hip.h -- one `inputs(seed)` / `call(t)` pair per header, defined once for both registries
(tests/test_gpu_stale_memory.py::CASES, which tests/test_gpu_bounds.py and tests/test_gpu_stream_order.py run again, and
tests/test_gpu_graph_replay.py::CASES) and for the restatement checks of tests/test_gpu_multiview.py, test_gpu_fit_views.py and
test_gpu_rig.py.  `inputs(seed)` -> {name: numpy array}; `call(t)` runs EVERY declaration of the header, host-only ones included,
on the device tensors `t` -> [(label, tensor)].  Nothing in rohm_amd/ imports this module."""
import numpy as np
import torch

import fit_views_ref as VR
import multiview_ref as MR
import rig_ref as RR
from rohm_amd.utils import synth

DEV = 'cuda:0'
_INPUTS, _CACHE = {}, {}


def _once(key, make):
    if key not in _INPUTS:
        _INPUTS[key] = make()
    return _INPUTS[key]


# ---- rohm_multiview.h: V = 4, N = 3, J = 22, salted inputs with one planted outlier per point ------------------------------------
MV_V, MV_N, MV_J = 4, 3, 22


def multiview_inputs(seed):
    """keypoints, cams, rigid, and world joints for the residuals (the restatement's, so that `rohm_mv_residuals` has an input of
    its own)."""
    def make():
        from rohm_amd.multiview import pack_cameras
        K, W, D = MR.make_rig(MV_V, seed, True)
        cams = pack_cameras(K, W, D)
        kp, _ = MR.make_views(cams, MV_N, MV_J, seed + 1, noise_px=2.0)
        kp = MR.salt(MR.plant_outliers(kp, 1, seed + 2)[0], seed + 3)
        rigid = np.concatenate([W[1, :3, :3].reshape(9), W[1, :3, 3]])
        return {'kp': kp, 'cams': cams, 'rigid': rigid, 'world': MR.triangulate(kp, cams)['joints']}
    return _once(('multiview', seed), make)


def multiview_call(t):
    from rohm_amd import multiview
    assert multiview.limits() == (16, 120)
    a = multiview.triangulate(t['kp'], t['cams'], rigid=t['rigid'], want_undistorted=True)
    b = multiview.triangulate(t['kp'], t['cams'], min_views=3, refine=1)               # rigid and keypoints_und NULL
    r = multiview.view_residuals(t['world'], t['kp'], t['cams'])
    return [('joints', a.joints), ('conf', a.conf), ('report', a.report), ('inliers', a.inliers), ('keypoints_und', a.keypoints_und),
            ('joints_world', b.joints), ('conf_3', b.conf), ('report_3', b.report), ('inliers_3', b.inliers), ('resid', r)]


# ---- rohm_fit_views.h: V = 3, N = 3, peppered inputs with an unusable middle frame, view 0 distorted, the start translation solved
# by the kernel; once with every optional operand (prev, resid, normal; robust, smoothed) and once with all three NULL (plain) ------
FV_V, FV_N = 3, 3
FV_SCALARS = ((700.0, 900.0, 30.0, 0.2, 3, 12), (0.0, 0.0, 0.0, 0.2, 2, 12))    # w_smooth, w_smooth_t, sigma_px, conf_min, iters, min_obs


def smplx_tensors():
    if 'tensors' not in _CACHE:
        _CACHE['tensors'] = synth.synthetic_smplx_tensors(0)
    return _CACHE['tensors']


def _nat():
    from rohm_amd.body_model import SMPLXLayer, native_for
    if 'layer' not in _CACHE:
        _CACHE['layer'] = SMPLXLayer.from_tensors(smplx_tensors()).to(DEV)
    return native_for(_CACHE['layer'], torch.device(DEV))


def fit_views_inputs(seed):
    def make():
        from rohm_amd.fit_views import default_w_prior
        cams = VR.make_rig(FV_V, seed, distorted=(0,))
        joints, truth, betas = VR.make_body(smplx_tensors(), FV_N, seed + 1, root_base=VR.facing(cams), root_angle=0.6, beta_scale=0.5)
        kp = VR.pepper(VR.make_keypoints(cams, joints, seed + 2, conf=(0.3, 1.0)), seed + 3, dead_frame=1)
        g = np.random.Generator(np.random.PCG64(seed + 4))
        init = truth.copy()
        init[:, :VR.NROT] += g.standard_normal((FV_N, VR.NROT)) * 0.05
        init[:, VR.NROT:] = np.nan
        return {'kp': kp, 'cams': cams, 'betas': np.repeat(betas[None].astype(np.float32), FV_N, axis=0), 'init': init,
                'prev': truth + 0.01, 'w_prior': default_w_prior(FV_V)}
    return _once(('fit_views', seed), make)


def fit_views_call(t):
    from rohm_amd.fit_views import fit_views_pose
    ws, wst, sigma, conf_min, iters, min_obs = FV_SCALARS[0]
    a = fit_views_pose(_nat(), t['kp'], t['cams'], t['betas'], t['init'], prev=t['prev'], w_prior=t['w_prior'], w_smooth=ws, w_smooth_t=wst,
                       sigma_px=sigma, conf_min=conf_min, iters=iters, min_obs=min_obs, want_normal=True)
    ws, wst, sigma, conf_min, iters, min_obs = FV_SCALARS[1]
    b = fit_views_pose(_nat(), t['kp'], t['cams'], t['betas'], t['init'], w_prior=t['w_prior'], sigma_px=sigma, conf_min=conf_min, iters=iters,
                       min_obs=min_obs, want_resid=False)                  # prev, resid and normal NULL
    return [('params', a[0]), ('report', a[1]), ('resid', a[2]), ('normal', a[3]), ('params_plain', b[0]), ('report_plain', b[1])]


# ---- rohm_rig.h: V = 4, N = 3, J = 22 (66 points: five tiles of the bundle adjustment, the last ragged), Q = 6 pairs, K = 5
# hypotheses; salted inputs with one planted outlier per point, a degenerate sample, a NaN point -----------------------------------
RIG_V, RIG_N, RIG_J, RIG_Q, RIG_K = 4, 3, 22, 6, 5
RIG_P = RIG_N * RIG_J


def rig_inputs(seed):
    """keypoints, the planted rig (disturbed), pairs, samples, the restatement's winning E, the planted points (disturbed, one NaN)
    and a camera step."""
    def make():
        from rohm_amd.multiview import pack_cameras
        V, N, J, Q, K, P = RIG_V, RIG_N, RIG_J, RIG_Q, RIG_K, RIG_P
        g = np.random.Generator(np.random.PCG64(seed + 9))
        Kc, W, D = MR.make_rig(V, seed, True, radius=3.0)
        cams = pack_cameras(Kc, W, D)
        kp, X = MR.make_views(cams, N, J, seed + 1, noise_px=2.0, spread=1.5)
        kp = MR.salt(MR.plant_outliers(kp, 1, seed + 2)[0], seed + 3)
        kp[1:, 1, :, 2] = 0.9                                              # salt() blinds frame 1; give it back to all but view 0
        cams[:, 9:12] += g.standard_normal((V, 3)) * 0.01
        pairs = np.stack(np.triu_indices(V, 1), 1).astype(np.int32)
        samples = RR.draw_samples(RR.undistorted(kp, cams), pairs, K, seed + 4, min_gap=4e-6)
        samples[0, 0, 3] = samples[0, 0, 1]                                # a repeated index
        ref = RR.pair_hypotheses(kp, cams, pairs, samples)
        E = np.stack([ref['E'][q, max(int(ref['best'][q]), 0)] for q in range(Q)])
        E[~np.isfinite(E).all(-1)] = 0.0
        points = X.reshape(P, 3) + g.standard_normal((P, 3)) * 0.01
        points[5] = np.nan
        return {'kp': kp, 'cams': cams, 'pairs': pairs, 'samples': samples, 'E': E, 'points': points, 'dc': g.standard_normal((V, 6)) * 1e-3}
    return _once(('rig', seed), make)


def rig_call(t):
    from rohm_amd import rig
    assert rig.pair_ws_bytes(RIG_V, RIG_P) == RIG_V * RIG_P * 16 and rig.ba_ws_bytes(RIG_V, RIG_P) > 0
    E, counts, best = rig.pair_hypotheses(t['kp'], t['cams'], t['pairs'], t['samples'])
    mom = rig.pair_moments(t['kp'], t['cams'], t['pairs'], t['E'])
    S, r, stats = rig.ba_moments(t['kp'], t['cams'], t['points'])
    Xn, cn = rig.ba_update(t['kp'], t['cams'], t['points'], t['dc'])
    return [('E_all', E), ('counts', counts), ('best', best), ('moments', mom), ('S', S), ('r', r), ('stats', stats), ('points_new', Xn),
            ('cams_new', cn)]


# case name ('family[variant]') -> (the header whose declarations the case runs, inputs, call)
CASES = {
    'multiview[V4, N3, J22]': ('rohm_multiview.h', multiview_inputs, multiview_call),
    'fit_views[V3, N3, dead middle frame]': ('rohm_fit_views.h', fit_views_inputs, fit_views_call),
    'rig[V4, N3, J22, Q6, K5]': ('rohm_rig.h', rig_inputs, rig_call),
}


def tensors(inputs, seed, put):
    """The value set `seed` as tensors, each handed to `put` (a registry's `_d`) as a fresh host copy."""
    return {k: put(torch.from_numpy(np.array(a))) for k, a in inputs(seed).items()}
