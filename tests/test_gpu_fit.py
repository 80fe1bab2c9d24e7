"""GPU: SMPL-X from 3-D joints -- `rohm_fit_pose` and `rohm_fit_shape_moments` (csrc/fit.hip) against their float64 restatement
(tests/fit_ref.py, held to finite differences and an independent forward kinematics in tests/test_fit_ref.py), `fit_joints` with
a shape, and `python -m rohm_amd.fit` end to end with the synthetic body layer.

Shapes: N = 1; N = 3 (smoothing at both ends, an invalid middle frame); N = 70 (more than a wave of frames and not a multiple of
one); confidences that are 0 or fractional, joints and whole frames of NaN.

Bars.  (a), (c), (d): kernel and restatement are both float64 on the same float32 inputs; they differ by the order of sums of at
most 66 products and by the device's sin / cos against the host's, a few ulp: about 1e-13 of the largest magnitude.  The bar is
1e-9 of each frame's largest |H|, of its largest |g|, of E, of a moments row's largest magnitude: four decades of margin.
(b): a near-tie in one accept / reject decision may take kernel and restatement down different, equally good paths, so the bars on
the final energies and on the fitted joints cannot be derived: they are ten times what was measured on an MI355X
(profiles/fit_parity.json: 'full_fit_energy_rel' and 'full_fit_joint_m').  Two conditions hold whatever was measured: E_end <=
E_start on every frame, and E_end(kernel) <= 1.05 E_end(restatement) on every frame."""
import json
import os

import numpy as np
import pytest
import torch

import fit_ref as FR
import stale_memory as SM
from rohm_amd.utils import synth

record = FR.record
pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NJ, NX, NROT = FR.NJ, FR.NX, FR.NROT
BAR = 1e-9
# ten times the largest values measured on an MI355X over the cases of test_full_fits (profiles/fit_parity.json)
ENERGY_BAR = 10 * 2.954e-13            # measured at N = 70: 2.954e-13 (N = 1: 1.6e-15, N = 3: 2.5e-15)
JOINT_BAR = 10 * 5.960e-08             # measured at N = 1: 5.960e-08 m, one float32 step of a joint (N = 3 and N = 70: 0)
FULL_ITERS = 20
FULL_CASES = ((1, 20), (3, 20), (70, 10))               # (N, iterations); 70 frames of the restatement take a second per four iterations

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


def w_prior():
    from rohm_amd.fit import default_w_prior
    return default_w_prior()


def run_pose(targets, conf, betas, init=None, prev=None, w_smooth=0.0, iters=FULL_ITERS, min_joints=6, want_normal=False):
    from rohm_amd.fit import fit_pose
    p, r, n = fit_pose(nat(), _dev(targets), _dev(conf), _dev(betas), init=_dev(init), prev=_dev(prev), w_prior=_dev(w_prior()),
                       w_smooth=w_smooth, iters=iters, min_joints=min_joints, want_normal=want_normal)
    return p.cpu().numpy(), r.cpu().numpy(), None if n is None else n.cpu().numpy()


def device_joints(params, betas):
    """`rohm_smplx_joints` of fitted parameters (float32, as a track stores them)."""
    from rohm_amd.export import _joints
    p = torch.from_numpy(params.astype(np.float32)).to(DEV)
    with torch.cuda.device(torch.device(DEV)):
        j = _joints(nat(), p[:, :NROT].reshape(-1, NJ, 3).contiguous(), _dev(betas.astype(np.float32)), p[:, NROT:].contiguous())
    return j.cpu().numpy().astype(np.float64)


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def problem(N, seed=None):
    """Frames with pose scale 0.3 rad, any root rotation, 1 cm of noise, a non-zero shape; on every second frame three limb or leaf
    joints are unobserved (confidence 0, a NaN position or a NaN confidence), the other confidences are fractional; where N
    allows, frame 1 is all NaN, frame 4 has 5 joints, frame 5 lacks a hip and frame 6 its neck."""
    key = ('problem', N)
    if key not in CACHE:
        g = np.random.Generator(np.random.PCG64(100 + N if seed is None else seed))
        joints, theta, transl, betas = FR.make_frames(tensors(), N, seed=200 + N, pose_scale=0.3, beta_scale=0.5, noise=0.01)
        conf = g.uniform(0.3, 1.0, size=(N, NJ)).astype(np.float32)
        limbs = np.array([4, 5, 7, 8, 10, 11, 15, 18, 19, 20, 21])
        for i in range(0, N, 2):
            a, b, c = g.choice(limbs, size=3, replace=False)
            conf[i, a] = 0.0
            joints[i, b, g.integers(0, 3)] = np.nan
            conf[i, c] = np.nan
        if N >= 3:
            joints[1] = np.nan
        if N >= 7:
            conf[4, 5:] = 0.0
            conf[5, 2] = -0.5
            joints[6, 12] = np.inf
        b = np.repeat(betas[None].astype(np.float32), N, axis=0)
        for a in (joints, conf, b):
            a.setflags(write=False)
        CACHE[key] = (joints, conf, b)
    return CACHE[key]


def reference(N, iters, want_normal=False):
    key = ('ref', N, iters, want_normal)
    if key not in CACHE:
        joints, conf, b = problem(N)
        CACHE[key] = FR.fit_pose(mdl(), joints, conf, b, w_prior=w_prior(), iters=iters, want_normal=want_normal)
    return CACHE[key]


# ---- (a) normal equations and the start point ------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', (1, 3, 70))
def test_normal_equations_match_the_restatement(N):
    joints, conf, b = problem(N)
    p_want, r_want, n_want = reference(N, 0, True)
    p, r, n = run_pose(joints, conf, b, iters=0, want_normal=True)
    assert p.shape == (N, NX) and r.shape == (N, 6) and n.shape == (N, NX, NX + 1)
    assert np.array_equal(r[:, 0], r_want[:, 0])
    if N >= 7:
        assert r_want[:7, 0].tolist() == [1, 0, 1, 1, 0, 2, 2]
    ok = r_want[:, 0] == 1
    assert not p[~ok].any() and not n[~ok].any() and np.isnan(r[~ok][:, [1, 2, 4, 5]]).all() and not r[~ok, 3].any()
    worst_h = worst_g = worst_e = 0.0
    for i in np.flatnonzero(ok):
        H, g, Hw, gw = n[i, :, :NX], n[i, :, NX], n_want[i, :, :NX], n_want[i, :, NX]
        assert np.array_equal(H, H.T)
        worst_h = max(worst_h, np.abs(H - Hw).max() / np.abs(Hw).max())
        worst_g = max(worst_g, np.abs(g - gw).max() / np.abs(gw).max())
        worst_e = max(worst_e, abs(r[i, 1] - r_want[i, 1]) / r_want[i, 1])
    start = np.abs(p - p_want).max()
    print(f'N={N}: H {worst_h:.3e}, g {worst_g:.3e}, E {worst_e:.3e} of the frame\'s largest (bar {BAR:.0e}); start point {start:.3e} (bar {BAR:.0e})')
    record('gpu', 'normal_H_rel', worst_h)
    record('gpu', 'normal_g_rel', worst_g)
    record('gpu', 'start_point_abs', start)
    assert worst_h <= BAR and worst_g <= BAR and worst_e <= BAR and start <= BAR
    assert np.array_equal(r[ok, 1], r[ok, 2]) and not r[:, 3].any() and (r[ok, 4] == FR.LAMBDA0).all()
    assert np.abs(r[ok, 5] - r_want[ok, 5]).max() <= BAR
    # the same input, the same bits; and without `normal` the rest is unchanged
    p2, r2, n2 = run_pose(joints, conf, b, iters=0, want_normal=True)
    assert p2.tobytes() == p.tobytes() and r2.tobytes() == r.tobytes() and n2.tobytes() == n.tobytes()
    p3, r3, _ = run_pose(joints, conf, b, iters=0)
    assert p3.tobytes() == p.tobytes() and r3.tobytes() == r.tobytes()


# ---- (b) full fits -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,iters', FULL_CASES, ids=lambda v: str(v))
def test_full_fits(N, iters):
    joints, conf, b = problem(N)
    p_want, r_want, _ = reference(N, iters)
    p, r, _ = run_pose(joints, conf, b, iters=iters)
    assert np.array_equal(r[:, 0], r_want[:, 0])
    ok = r_want[:, 0] == 1
    assert not p[~ok].any()
    e_rel = np.abs(r[ok, 2] - r_want[ok, 2]) / r_want[ok, 2]
    jd = np.linalg.norm(device_joints(p[ok], b[ok]) - device_joints(p_want[ok], b[ok]), axis=-1)
    ratio = r[ok, 2] / r_want[ok, 2]
    print(f'N={N}, {iters} iterations, {int(ok.sum())} frames fitted: |E_end - restatement| / E_end max {e_rel.max():.3e} (bar {ENERGY_BAR:.3e}), '
          f'joints of the fitted parameters max {jd.max():.3e} m (bar {JOINT_BAR:.3e}); E_end / restatement in [{ratio.min():.6f}, {ratio.max():.6f}]; '
          f'accepted {r[ok, 3].min():.0f} .. {r[ok, 3].max():.0f}, E_end / E_start max {(r[ok, 2] / r[ok, 1]).max():.3e}, rms max {r[ok, 5].max() * 1e3:.2f} mm')
    record('gpu', 'full_fit_energy_rel', e_rel.max())
    record('gpu', 'full_fit_joint_m', jd.max())
    record('gpu', 'full_fit_energy_ratio_max', ratio.max())
    assert (r[ok, 2] <= r[ok, 1]).all()
    assert (r[ok, 2] <= 1.05 * r_want[ok, 2]).all()
    assert (r[ok, 3] >= 1).all() and (r[ok, 3] <= iters).all()
    assert e_rel.max() <= ENERGY_BAR
    assert jd.max() <= JOINT_BAR


# ---- (c) smoothing -------------------------------------------------------------------------------------------------------------------
def test_smoothing_term_and_frames_without_neighbours():
    joints, conf, b = problem(3)
    base, rb, _ = reference(3, FULL_ITERS)
    assert rb[:, 0].tolist() == [1, 0, 1]
    # three frames that all have a fit: the middle one from frame 0's joints
    j3, c3 = joints.copy(), conf.copy()
    j3[1], c3[1] = joints[0], conf[0]
    sol = base.copy()
    sol[1] = base[0] + 0.01
    for prev, label in ((sol, 'both neighbours'), (np.where(np.arange(3)[:, None] == 2, np.nan, sol), 'one neighbour')):
        p, r, _ = run_pose(j3, c3, b, init=sol, prev=prev, w_smooth=0.05, iters=0)
        pw, rw, _ = FR.fit_pose(mdl(), j3, c3, b, init=sol, prev=prev, w_prior=w_prior(), w_smooth=0.05, iters=0)
        plain = run_pose(j3, c3, b, init=sol, iters=0)[1]
        rel = np.abs(r[:, 1] - rw[:, 1]).max() / rw[:, 1].max()
        print(f'{label}: E with the smoothing term against the restatement {rel:.3e} (bar {BAR:.0e}); the term itself {r[:, 1] - plain[:, 1]}')
        record('gpu', 'smoothing_energy_rel', rel)
        assert rel <= BAR and np.array_equal(p, sol)
        assert r[1, 1] > plain[1, 1]
    assert r[0, 1] > plain[0, 1] and r[1, 1] > plain[1, 1] and r[2, 1] > plain[2, 1]      # (the last loop: frame 1 sees frame 0, frame 2 sees frame 1)
    # the smoothed fit against the restatement's, same iterations: the two conditions of (b)
    p, r, _ = run_pose(j3, c3, b, init=sol, prev=sol, w_smooth=0.05, iters=FULL_ITERS)
    pw, rw, _ = FR.fit_pose(mdl(), j3, c3, b, init=sol, prev=sol, w_prior=w_prior(), w_smooth=0.05, iters=FULL_ITERS)
    assert (r[:, 2] <= r[:, 1]).all() and (r[:, 2] <= 1.05 * rw[:, 2]).all()
    # frames without a finite neighbour: the unsmoothed fit, bit for bit.  Frame 1 is invalid (a NaN row), so 0 and 2 have none.
    prev = np.where(np.arange(3)[:, None] == 1, np.nan, base)
    init = prev.copy()
    a = run_pose(joints, conf, b, init=init, prev=prev, w_smooth=0.5, iters=5)
    c = run_pose(joints, conf, b, init=init, iters=5)
    assert a[1][:, 0].tolist() == [1, 0, 1] and a[0].tobytes() == c[0].tobytes() and a[1].tobytes() == c[1].tobytes()
    # N = 1 has no neighbour at all
    one = run_pose(joints[:1], conf[:1], b[:1], init=base[:1], prev=base[:1], w_smooth=0.5, iters=5)
    assert one[0].tobytes() == run_pose(joints[:1], conf[:1], b[:1], init=base[:1], iters=5)[0].tobytes()


# ---- (d) shape moments ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', (1, 3, 70))
def test_shape_moments_match_the_restatement(N):
    from rohm_amd.fit import shape_moments
    joints, conf, b = problem(N)
    g = np.random.Generator(np.random.PCG64(300 + N))
    params = np.concatenate([g.standard_normal((N, NROT)) * 0.3, g.standard_normal((N, 3)) + (0, 0, 3.0)], axis=1)
    use = (np.arange(N) % 5 != 2).astype(np.uint8)
    rows_want, out_want = FR.shape_moments(mdl(), joints, conf, params, use)
    rows, out = shape_moments(nat(), _dev(joints), _dev(conf), _dev(params), _dev(use))
    rows2, out2 = shape_moments(nat(), _dev(joints), _dev(conf), _dev(params), _dev(use.astype(bool)))
    assert torch.equal(rows.view(torch.int64), rows2.view(torch.int64)) and torch.equal(out.view(torch.int64), out2.view(torch.int64))
    rows, out = rows.cpu().numpy(), out.cpu().numpy()
    assert rows.shape == (N, 66) and out.shape == (66,) and not rows[use == 0].any()
    scale = np.maximum(np.abs(rows_want).max(axis=1, keepdims=True), 1e-300)
    rel_rows = (np.abs(rows - rows_want) / scale).max()
    rel_out = np.abs(out - out_want).max() / max(np.abs(out_want).max(), 1e-300)
    print(f'N={N}: per-frame rows {rel_rows:.3e}, totals {rel_out:.3e} of the largest magnitude (bar {BAR:.0e})')
    record('gpu', 'moments_rows_rel', rel_rows)
    record('gpu', 'moments_total_rel', rel_out)
    assert rel_rows <= BAR and rel_out <= BAR
    if N >= 3:
        assert use[1] and not rows_want[1].any() and not rows[1].any()                  # frame 1 is all NaN: every c is 0


# ---- (e) one shape for the recording ----------------------------------------------------------------------------------------------------
def test_fit_joints_with_a_shape():
    from rohm_amd.fit import fit_joints
    joints, _, _, betas = FR.make_frames(tensors(), 12, seed=41, pose_scale=0.15, beta_scale=1.0, noise=0.002, walk=True)
    res = fit_joints(joints, fit_shape=True, shape_rounds=3, iters=10, smooth_passes=1, body_model=_layer(), device=DEV)
    h = res.energy_history
    zero = fit_joints(joints, fit_shape=False, iters=10, smooth_passes=0, body_model=_layer(), device=DEV)
    e_zero = float(zero.report[zero.valid, 2].sum())
    print(f'energy history {h}; the fit with beta = 0: {e_zero:.6e}; betas fitted {np.round(res.betas, 3)} against {np.round(betas, 3)}')
    assert res.valid.all() and len(h) == 4
    assert all(h[i + 1] <= h[i] * (1 + 1e-12) for i in range(3))                        # float64 sums of 12 energies: 1e-12 is their rounding
    assert h[0] == pytest.approx(e_zero, rel=1e-12) and h[-1] < e_zero
    assert res.betas.any() and not zero.betas.any() and zero.energy_history is None


# ---- (f) end to end -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def body_dir(tmp_path_factory):
    """SMPLX_NEUTRAL.npz in the released layout from the synthetic model."""
    t = tensors()
    V = t['v_template'].shape[0]
    kt = np.stack([np.array(synth.SMPLX_PARENTS), np.arange(55)]).astype(np.int64)
    kt[0, 0] = 2 ** 32 - 1
    d = tmp_path_factory.mktemp('body')
    np.savez(str(d / 'SMPLX_NEUTRAL.npz'), v_template=t['v_template'].numpy(), shapedirs=t['shapedirs'].numpy(),
             posedirs=t['posedirs'].numpy().T.reshape(V, 3, 486), J_regressor=t['J_regressor'].numpy(), kintree_table=kt,
             weights=t['lbs_weights'].numpy(), f=np.zeros((4, 3), np.int64))
    return str(d)


GAPS = (0, 7, 8, 22, 39)


def test_cli_from_a_body25_file_to_a_track(tmp_path, body_dir, capsys):
    """N = 40 frames of a walking synthetic body as a BODY_25 file with five detector gaps -> `python -m rohm_amd.fit` -> a track that
    `read_track` accepts, `valid` false at the gaps, and whose joints (`floor.track_joints`, float32) are the input's at the
    observed joints.

    Two runs.  With the default options the fit is regularised: the prior and the smoothing pull it off noise-free joints by
    their bias (measured: 1.8 mm at most, 0.23 mm in the median; five spine and collar joints are unobserved in a BODY_25 file, so the
    prior has more to say than in the recovery check of tests/test_fit_ref.py).  It is held to 5 mm: half of the 1 cm of noise that
    the defaults are meant for (the noise of test_full_fits), so that regularising never costs more than it can gain.  The bar of test_full_fits (6e-7 m, a few float32 steps of a joint) is met by the fit without that
    bias, `--prior_scale 0 --w_smooth 0`, of a body near the origin of its frame of reference, where a float32 step of a joint is
    6e-8 m (measured: 1.4e-7 m at most; 3 m in front of a camera, where the step is 2.4e-7 m, 4.9e-7 m)."""
    from rohm_amd.data_loaders.dataloader_video import OPENPOSE_TO_SMPL
    from rohm_amd.data_loaders.track import TRACK_KEYS, read_track
    from rohm_amd.fit import BODY25_PROXY, main
    from rohm_amd.floor import track_joints
    N = 40
    joints = FR.make_frames(tensors(), N, seed=51, pose_scale=0.12, walk=True, centre=(0.0, 0.0, 0.0))[0]
    j25, c25 = np.zeros((N, 25, 3), np.float32), np.zeros((N, 25), np.float32)
    observed = [s for s in range(NJ) if s not in BODY25_PROXY]
    for s in observed:
        j25[:, OPENPOSE_TO_SMPL[s]] = joints[:, s]
        c25[:, OPENPOSE_TO_SMPL[s]] = 1.0
    j25[list(GAPS)] = np.nan
    c25[list(GAPS)] = 0.0
    want_valid = np.ones(N, bool)
    want_valid[list(GAPS)] = False
    skel, js = str(tmp_path / 'skeleton.npz'), str(tmp_path / 'report.json')
    np.savez(skel, joints_3d=j25, joint_conf=c25, fps=30.0, cam2world=np.eye(4), recording_name=np.array('walk'))
    for label, opts, bar in (('default options', [], 5e-3), ('no prior, no smoothing', ['--prior_scale', '0', '--w_smooth', '0'], JOINT_BAR)):
        out = str(tmp_path / ('track_%d.npz' % len(opts)))
        assert main(['--skeleton', skel, '--out', out, '--body_model_path', body_dir, '--json', js, '--device', DEV] + opts) == 0
        text = capsys.readouterr().out
        assert 'pass 1:' in text and 'smoothing pass 1' in text and 'frames fitted / skipped:     35 / 5 of 40' in text and 'wrote' in text
        with np.load(out, allow_pickle=False) as f:
            track = {k: f[k] for k in f.files}
        assert set(track) <= set(TRACK_KEYS) and {'global_orient', 'transl', 'body_pose', 'betas', 'valid', 'fps', 'cam2world', 'recording_name'} == set(track)
        rec = read_track(out)
        assert np.array_equal(rec['valid'], want_valid) and np.array_equal(track['valid'], want_valid)
        with open(js) as f:
            rep = json.load(f)
        assert rep['summary']['fitted'] == 35 and rep['summary']['skipped'] == 5 and len(rep['report']) == N
        assert rep['options']['prior_scale'] == (0.0 if opts else 1.0)
        _, _, fitted = track_joints(out, body_dir, DEV)
        d = np.linalg.norm(fitted.cpu().numpy().astype(np.float64)[want_valid][:, observed] - joints.astype(np.float64)[want_valid][:, observed], axis=-1)
        print(f'end to end, {label}: fitted joints against the input at the observed joints: max {d.max():.3e} m, median {np.median(d):.3e} m '
              f'(bar {bar:.3e}); median residual {rep["summary"]["median_residual_m"]:.3e} m')
        record('gpu', 'end_to_end_joint_m' + ('_no_prior' if opts else ''), d.max())
        assert d.max() <= bar


# ---- (g) stale memory ---------------------------------------------------------------------------------------------------------------------
def _all_outputs():
    from rohm_amd.fit import fit_pose, shape_moments
    joints, conf, b = problem(70)
    base = reference(70, 0)[0]
    sol = np.where(reference(70, 0)[1][:, :1] == 1, base, np.nan)
    p, r, n = fit_pose(nat(), _dev(joints), _dev(conf), _dev(b), w_prior=_dev(w_prior()), iters=3, want_normal=True)
    p2, r2, _ = fit_pose(nat(), _dev(joints), _dev(conf), _dev(b), init=_dev(sol), prev=_dev(sol), w_prior=_dev(w_prior()), w_smooth=0.01, iters=2)
    rows, out = shape_moments(nat(), _dev(joints), _dev(conf), _dev(base), _dev((np.arange(70) % 3 != 0).astype(np.uint8)))
    torch.cuda.synchronize()
    return [('params', p), ('report', r), ('normal', n), ('params_smooth', p2), ('report_smooth', r2), ('moment_rows', rows), ('moments', out)]


def test_outputs_do_not_depend_on_what_their_memory_held():
    with SM.poison(SM.ZEROS):
        want = _all_outputs()
    for name, word in SM.PATTERNS.items():
        with SM.poison(word):
            got = _all_outputs()
        for (label, a), (_, b) in zip(want, got):
            assert SM.first_difference(a, b) is None, (name, label, SM.first_difference(a, b))


# ---- bad arguments --------------------------------------------------------------------------------------------------------------------------
def test_kernels_refuse_bad_arguments():
    from rohm_amd import _lib
    from rohm_amd.fit import fit_pose, shape_moments
    lib, stream = _lib.lib(), _lib.stream_ptr(torch.device(DEV))
    joints, conf, b = (_dev(a) for a in problem(3))
    wp = _dev(w_prior())
    params, report = torch.empty(3, NX, device=DEV, dtype=torch.float64), torch.empty(3, 6, device=DEV, dtype=torch.float64)
    h = nat().handle

    def pose(N=3, iters=1, min_joints=6, w_smooth=0.0, targets=joints.data_ptr(), handle=h):
        return lib.rohm_fit_pose(handle, targets, conf.data_ptr(), b.data_ptr(), None, None, wp.data_ptr(), w_smooth, iters, min_joints, N,
                                 params.data_ptr(), report.data_ptr(), None, stream)
    assert pose() == 0 and pose(N=0, targets=None, handle=None) == 0
    assert pose(N=-1) == -1 and b'N must be' in lib.rohm_last_error()
    assert pose(iters=-1) == -1 and b'iters' in lib.rohm_last_error()
    assert pose(min_joints=0) == -1 and pose(min_joints=23) == -1 and b'min_joints' in lib.rohm_last_error()
    assert pose(w_smooth=float('nan')) == -1 and b'w_smooth' in lib.rohm_last_error()
    assert pose(targets=None) == -1 and b'null' in lib.rohm_last_error()
    rows, out = torch.empty(3, 66, device=DEV, dtype=torch.float64), torch.empty(66, device=DEV, dtype=torch.float64)
    use = torch.ones(3, device=DEV, dtype=torch.uint8)

    def mom(N=3, targets=joints.data_ptr()):
        return lib.rohm_fit_shape_moments(h, targets, None, params.data_ptr(), use.data_ptr(), N, rows.data_ptr(), out.data_ptr(), stream)
    assert mom() == 0 and mom(N=0, targets=None) == 0
    assert mom(N=-1) == -1 and b'N must be' in lib.rohm_last_error()
    assert mom(targets=None) == -1 and b'null' in lib.rohm_last_error()
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match=r'\[N, 22, 3\]'):
        fit_pose(nat(), joints[:, :21], conf, b)
    with pytest.raises(ValueError, match=r'betas must be'):
        fit_pose(nat(), joints, conf, b[:2])
    with pytest.raises(ValueError, match=r'init must be'):
        fit_pose(nat(), joints, conf, b, init=params[:, :66])
    with pytest.raises(ValueError, match=r'use must be'):
        shape_moments(nat(), joints, conf, params, use[:2])
    with pytest.raises(_lib.RohmHipError):
        fit_pose(nat(), joints.cpu(), None, b)
