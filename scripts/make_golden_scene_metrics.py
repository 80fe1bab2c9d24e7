"""Golden vectors of the PROX / EgoBody evaluation -> tests/golden/scene_metrics.npz (and the AMASS pickle-path lines).

What oracle/make_golden.py::golden_metrics does for eval_amass_full.py, done for eval_prox_egobody.py: the script
cannot be imported (argparse, smplx, open3d, pyrender, cv2 at module level), so its statement blocks are read from the
file and executed on synthetic driver results -- the per-recording block :172-272 (contact labels, back to scene
coordinates, skating, acceleration, MPJPE, ground penetration) and the final block :453-490 with `print` captured.
`points_coord_trans` comes from the reference's utils.other_utils through oracle.refload (which stubs cv2).

The synthetic joint tracks are generated on a 2^-10 m grid and stored as int8 steps; the canonical float32 joints are
derived from them (tests/scene_metrics_ref.py::cano_from_scene), which keeps the fixture small.

Needs a RoHM checkout at oracle.refload.REF_ROOT; run once where it exists, commit only the .npz:
    python scripts/make_golden_scene_metrics.py
"""
import os
import sys
import textwrap
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle import refload  # noqa: E402
import scene_metrics_ref as R  # noqa: E402  (the fixture's encoding)

OUT = os.path.join(ROOT, 'tests', 'golden', 'scene_metrics.npz')
UP = {'prox': 2, 'egobody': 1}
# synthetic scenes (no floor-height table of the reference is reproduced here)
RECORDINGS = {'prox': [('N0Sofa_00034_01', 'N0Sofa', -0.9130859375 - 1e-4, 1), ('MPH1Library_00034_01', 'MPH1Library', -0.3427, 2)],
              'egobody': [('recording_20210907_S02_S01_01', 'seminar_g110', -1.6537, 2),
                          ('recording_20220315_S21_S30_03', 'seminar_d78', -0.8125, 1)]}
T, T_GT = 143, 144
GRID = R.GRID


def _rot(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * k @ k


def synthetic_recording(g, n, up, ground, family):
    """Scene-coordinate joints walking over a floor at `ground` (feet sliding near it, toes below it) and their GT, both
    on the 2^-10 m grid (int), a mask with ~30 % occluded joints, and trans_scene2cano of the given family:
      general: tilted rotation + translation (float32 matrix; the back-transform is inexact)
      exact:   rotation by a multiple of 90 deg about the up axis, translation on the grid, so the float32 inverse and
               the transform are exact."""
    horiz = [0, 1] if up == 2 else [0, 2]
    gt = np.zeros((n, T_GT, 22, 3))
    root = np.cumsum(g.normal(0, 0.003, (n, T_GT, 3)), axis=1) + g.uniform(-2, 2, (n, 1, 3))
    gt += root[:, :, None, :] + g.normal(0, 0.25, (n, 1, 22, 3))
    gt[..., up] = ground + 0.2 + np.cumsum(g.normal(0, 0.001, (n, T_GT, 22)), axis=1) + \
        np.abs(g.normal(0.7, 0.4, (n, 1, 22)))
    for f, (lo, hi) in ((7, (0.0, 0.17)), (8, (0.0, 0.17)), (10, (-0.09, 0.12)), (11, (-0.09, 0.12))):
        phase = g.uniform(0, 2 * np.pi, (n, 1)) + np.cumsum(g.normal(0, 0.3, (n, T_GT)), axis=1)
        gt[:, :, f, up] = ground + lo + (hi - lo) * (0.5 + 0.5 * np.sin(phase))     # lifts and sets down the foot
        step = 0.005 + 0.004 * np.sin(g.uniform(0, 2 * np.pi, (n, 1)) + np.cumsum(g.normal(0, 0.4, (n, T_GT)), axis=1))
        ang = g.uniform(0, 2 * np.pi, (n, 1)) + np.cumsum(g.normal(0, 0.3, (n, T_GT)), axis=1)   # slide, 0.03-0.27 m/s
        gt[:, :, f, horiz[0]] = gt[:, 0:1, f, horiz[0]] + np.cumsum(step * np.cos(ang), axis=1)
        gt[:, :, f, horiz[1]] = gt[:, 0:1, f, horiz[1]] + np.cumsum(step * np.sin(ang), axis=1)
    rec = gt[:, :T] + g.normal(0, 0.01, (n, 1, 22, 3)) + np.cumsum(g.normal(0, 0.0008, (n, T, 22, 3)), axis=1)
    rec[:, :, [10, 11], up] -= 0.015 + 0.015 * np.sin(g.uniform(0, 6.3, (n, 1, 2)) +
                                                      np.cumsum(g.normal(0, 0.3, (n, T, 2)), axis=1))
    mask = g.uniform(size=(n, T, 22)) > 0.3
    m = np.tile(np.eye(4), (n, 1, 1))
    for i in range(n):
        if family == 'exact':
            m[i, :3, :3] = np.round(_rot(np.eye(3)[up], g.integers(0, 4) * np.pi / 2))
            m[i, :3, 3] = np.round(g.uniform(-3, 3, 3) / GRID) * GRID
        else:
            m[i, :3, :3] = _rot(g.normal(size=3), g.uniform(0.3, 2.5))
            m[i, :3, 3] = g.uniform(-3, 3, 3)
    q = lambda a: np.round(a / GRID).astype(np.int64)
    return q(rec), m.astype(np.float32), q(gt), mask


def main():
    if not refload.available():
        raise SystemExit(f'needs the reference checkout at {refload.REF_ROOT}')
    ref = refload.load()
    src = open(os.path.join(refload.REF_ROOT, 'eval_prox_egobody.py')).read().split('\n')
    assert src[171].strip().startswith('################ get contact lbls') and src[452].strip().startswith('#####')
    per_rec = compile(textwrap.dedent('\n'.join(src[171:272])), 'eval_prox_egobody.py[172:272]', 'exec')
    final = compile(textwrap.dedent('\n'.join(src[452:490])), 'eval_prox_egobody.py[453:490]', 'exec')
    out = {}
    for seed_base, family in ((100, 'general'), (200, 'exact')):
        for di, dataset in enumerate(('prox', 'egobody')):
            g = np.random.Generator(np.random.PCG64(seed_base + di))
            key = f'{dataset}_{family}'
            ns = {'np': np, 'points_coord_trans': ref.other_utils.points_coord_trans,
                  'args': types.SimpleNamespace(dataset=dataset),
                  'prox_floor_height': {}, 'egobody_floor_height': {}}
            for name in ('skating_list', 'acc_list', 'acc_error_list', 'ground_pene_dist_list', 'ground_pene_freq_list',
                         'gmpjpe_list', 'mpjpe_list', 'mpjpe_list_vis', 'mpjpe_list_occ', 'joint_mask_list'):
                ns[name] = {}
            names = []
            for ri, (rec_name, scene, ground, n) in enumerate(RECORDINGS[dataset]):
                rec_q, m, gt_q, mask_bool = synthetic_recording(g, n, UP[dataset], ground, family)
                rec = R.cano_from_scene(rec_q * GRID, m)             # what the driver pickles (canonical, float32)
                gt = (gt_q * GRID).astype(np.float32)
                mask = mask_bool.astype(np.float32)
                ns[f'{dataset}_floor_height'][scene] = ground
                ns.update(recording_name=rec_name, scene_name=scene, n_seq=n, clip_len_rec=T,
                          trans_scene2cano_list=m.copy(), rec_ric_data_rec_list_from_smpl=rec.copy(),
                          rec_ric_data_noisy_list=rec.copy(), motion_repr_rec_list=np.zeros((n, T, 294), np.float32),
                          mask_joint_vis_list=mask.copy(),
                          joints_gt_scene_coord_list=gt[:, 0:T] if dataset == 'egobody' else None)   # :170
                exec(per_rec, ns)
                p = f'{key}_{ri}_'
                out[p + 'name'], out[p + 'ground_height'] = np.str_(rec_name), np.float64(ground)
                (out[p + 'gt_first'], out[p + 'gt_steps']), out[p + 'trans_scene2cano'] = R.encode_track(gt_q), m
                (out[p + 'rec_first'], out[p + 'rec_steps']) = R.encode_track(rec_q - gt_q[:, :T])
                if dataset == 'egobody':
                    out[p + 'mask_bits'], out[p + 'mask_shape'] = np.packbits(mask_bool.reshape(-1)), np.array(mask.shape)
                names.append(rec_name)
            ns['test_recording_name_list'] = names
            lines = []
            ns['print'] = lambda *a, **k: lines.append(' '.join(str(x) for x in a))
            exec(final, ns)
            for ri, rec_name in enumerate(names):
                p = f'{key}_{ri}_'
                arrays = {'skating': ns['skating_list'][rec_name], 'acc': ns['acc_list'][rec_name],
                          'pene_freq': ns['ground_pene_freq_list'][rec_name],
                          'pene_dist': ns['ground_pene_dist_list'][rec_name]}
                if dataset == 'egobody':
                    arrays.update(acc_error=ns['acc_error_list'][rec_name], gmpjpe=ns['gmpjpe_list'][rec_name],
                                  mpjpe=ns['mpjpe_list'][rec_name], mpjpe_vis=ns['mpjpe_list_vis'][rec_name],
                                  mpjpe_occ=ns['mpjpe_list_occ'][rec_name])
                out.update(R.encode_arrays(arrays, p))
            out[key + '_n_recordings'] = np.int64(len(names))
            out[key + '_lines'] = np.array(lines)
            a = lambda k: ns[k]['all']
            vals = {'skating': a('skating_list').mean(), 'ground_pene_freq': a('ground_pene_freq_list').mean() * 100,
                    'ground_pene_dist': -a('ground_pene_dist_list').mean() * 1000}
            if dataset == 'prox':
                vals['acc'] = a('acc_list').mean()
            else:
                vals.update(acc_error=a('acc_error_list').mean(), gmpjpe=a('gmpjpe_list').mean() * 1000,
                            mpjpe=a('mpjpe_list').mean() * 1000,
                            mpjpe_vis=a('mpjpe_list_vis').sum() / a('joint_mask_list').sum() * 1000,
                            mpjpe_occ=a('mpjpe_list_occ').sum() / (1 - a('joint_mask_list')).sum() * 1000)
            for k, v in vals.items():
                out[f'{key}_value_{k}'] = np.float64(v)
            print(key, lines)

    # AMASS pickle path: the lines eval_amass_full.py:72-147 prints on oracle.metrics.synthetic_results(5)
    from oracle import metrics as M
    asrc = open(os.path.join(refload.REF_ROOT, 'eval_amass_full.py')).read().split('\n')
    assert asrc[71].strip().startswith('joints_mpjpe_global')
    block = compile(textwrap.dedent('\n'.join(asrc[71:147])), 'eval_amass_full.py[72:147]', 'exec')
    clean, rec, r_clean, r_rec = M.synthetic_results(5)
    lines = []
    ns = {'np': np, 'args': types.SimpleNamespace(mask_scheme='lower', traj_mask_ratio=0.0),
          'rec_ric_data_clean_list': clean, 'rec_ric_data_rec_list_from_smpl': rec, 'motion_repr_rec_list': r_rec.copy(),
          'motion_repr_clean_list': r_clean.copy(), 'n_seq': len(clean), 'clip_len': clean.shape[1],
          'print': lambda *a, **k: lines.append(' '.join(str(x) for x in a))}
    exec(block, ns)
    out['amass_results_seed'], out['amass_mask_scheme'], out['amass_lines'] = np.int64(5), np.str_('lower'), np.array(lines)
    print('amass', lines)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT))


if __name__ == '__main__':
    main()
