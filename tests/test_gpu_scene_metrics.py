"""GPU: rohm_scene_metrics / rohm_amd.evaluation (PROX / EgoBody, eval_prox_egobody.py:172-270) against the reference's
own statements (tests/golden/scene_metrics.npz) and the numpy restatement (tests/scene_metrics_ref.py), and the headless
evaluator end to end on driver pickles."""
import math
import pickle

import numpy as np
import pytest
import torch

import scene_metrics_ref as R
from helpers import golden
from oracle import metrics as M
from rohm_amd import evaluation as E

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GRID = 2.0 ** -10
COUNTS = ('skating', 'ground_pene_freq')


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _device_metrics(case, dataset):
    parts = [E.scene_metrics(_dev(r['joints_rec']), _dev(r['trans_scene2cano']), r['ground_height'], dataset,
                             joints_gt=_dev(r['joints_gt']), mask_joint_vis=_dev(r['mask'])) for r in case]
    return parts[0].merge(*parts[1:])


def _exact_clips(seed, B, T, dataset, T_gt=None):
    """Clips whose back-transform is exact (coordinates / translations on a 2^-10 m grid, rotations by multiples of 90 deg
    about the up axis): the device's float32 elements are then bit-identical to numpy's."""
    g = np.random.Generator(np.random.PCG64(seed))
    up = R.UP[dataset]
    T_gt = T_gt or T + 1
    ground = -0.75 - 0.001 * seed
    gt = g.normal(0, 0.4, (B, 1, 22, 3)) + np.cumsum(g.normal(0, 0.006, (B, T_gt, 22, 3)), axis=1)
    gt[..., up] = ground + np.abs(g.normal(0.5, 0.4, (B, T_gt, 22)))
    gt[:, :, R.FOOT, up] = ground + g.uniform(-0.08, 0.2, (B, T_gt, 4))
    gt = np.round(gt / GRID) * GRID
    rec = np.round((gt[:, :T] + g.normal(0, 0.01, (B, T, 22, 3))) / GRID) * GRID
    m = np.tile(np.eye(4), (B, 1, 1))
    for i in range(B):
        c, s = [(1, 0), (0, 1), (-1, 0), (0, -1)][g.integers(0, 4)]
        a, b = [k for k in range(3) if k != up]
        m[i, a, a], m[i, a, b], m[i, b, a], m[i, b, b] = c, -s, s, c
        m[i, :3, 3] = np.round(g.uniform(-2, 2, 3) / GRID) * GRID
    cano = np.einsum('ntjc,nrc->ntjr', rec, m[:, :3, :3]) + m[:, None, None, :3, 3]
    mask = (g.uniform(size=(B, T, 22)) > 0.3).astype(np.float32)
    f = lambda x: np.ascontiguousarray(x, dtype=np.float32)
    return f(cano), f(m), ground, f(gt), mask


@pytest.mark.parametrize('dataset', ['prox', 'egobody'])
@pytest.mark.parametrize('family', ['exact', 'general'])
def test_summary_vs_reference_golden(dataset, family):
    g = golden('scene_metrics.npz')
    case = R.golden_case(g, dataset, family)
    out = _device_metrics(case, dataset).summary()
    near_sk = near_pe = 0
    if family == 'general':
        for r in case:
            a, b = R.near_threshold(r['joints_rec'], r['trans_scene2cano'], r['ground_height'], dataset)
            near_sk, near_pe = near_sk + a, near_pe + b
    n = sum(len(r['joints_rec']) for r in case)
    T = case[0]['joints_rec'].shape[1]
    for k, v in out.items():
        ref = float(g[f'{dataset}_{family}_value_{k}'])
        if k == 'skating':
            assert abs(round(v * n * (T - 1)) - round(ref * n * (T - 1))) <= near_sk, (k, v, ref, near_sk)
        elif k == 'ground_pene_freq':
            assert abs(round(v / 100 * n * 2 * T) - round(ref / 100 * n * 2 * T)) <= near_pe, (k, v, ref, near_pe)
        else:
            assert abs(v - ref) <= (1e-6 if family == 'exact' else 1e-5) * abs(ref), (k, v, ref)
    if family == 'exact':
        assert E.SceneMetrics(dataset, T, np.concatenate([_device_metrics([r], dataset).sums for r in case])).lines() == \
            list(g[f'{dataset}_{family}_lines'])


@pytest.mark.parametrize('dataset', ['prox', 'egobody'])
@pytest.mark.parametrize('B', [1, 32, 64])
@pytest.mark.parametrize('T', [3, 16, 143, 255])
def test_clip_sums_vs_restatement(dataset, B, T):
    cano, m, ground, gt, mask = _exact_clips(B * 1000 + T, B, T, dataset)
    gt_in = gt if dataset == 'egobody' else None
    mask_in = mask if dataset == 'egobody' else None
    got = E.scene_metrics(_dev(cano), _dev(m), ground, dataset, joints_gt=_dev(gt_in), mask_joint_vis=_dev(mask_in)).sums
    ref = R.clip_sums(cano, m, ground, dataset, gt_in, mask_in)
    assert got.shape == (B, 11)
    np.testing.assert_array_equal(got[:, [0, 3, 8, 10]], ref[:, [0, 3, 8, 10]])        # counts and mask sums
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12)


def test_joints_scene_vs_points_coord_trans():
    g = golden('scene_metrics.npz')
    for dataset in ('prox', 'egobody'):
        for r in R.golden_case(g, dataset, 'general'):
            _, js = E.scene_metrics(_dev(r['joints_rec']), _dev(r['trans_scene2cano']), r['ground_height'], dataset,
                                    joints_gt=_dev(r['joints_gt']), mask_joint_vis=_dev(r['mask']), return_joints_scene=True)
            ref = R.to_scene(r['joints_rec'], r['trans_scene2cano'])
            assert np.abs(js.cpu().numpy() - ref).max() <= 1e-5


def test_split_batch_merge_equals_one_call():
    cano, m, ground, gt, mask = _exact_clips(7, 40, 143, 'egobody', T_gt=150)
    one = E.scene_metrics(_dev(cano), _dev(m), ground, 'egobody', _dev(gt), _dev(mask))
    a = E.scene_metrics(_dev(cano[:13]), _dev(m[:13]), ground, 'egobody', _dev(gt[:13]), _dev(mask[:13]))
    b = E.scene_metrics(_dev(cano[13:]), _dev(m[13:]), ground, 'egobody', _dev(gt[13:]), _dev(mask[13:]))
    merged = a.merge(b)
    assert np.array_equal(merged.sums, one.sums)
    assert merged.summary() == one.summary()


def test_all_visible_mask_gives_nan_occ():
    cano, m, ground, gt, mask = _exact_clips(3, 4, 16, 'egobody')
    out = E.scene_metrics(_dev(cano), _dev(m), ground, 'egobody', _dev(gt), _dev(np.ones_like(mask))).summary()
    assert math.isnan(out['mpjpe_occ']) and out['mpjpe_vis'] == pytest.approx(out['mpjpe'], rel=1e-12)


def test_bad_arguments_raise():
    cano, m, ground, gt, mask = _exact_clips(4, 2, 16, 'egobody')
    j, t, g_, k = _dev(cano), _dev(m), _dev(gt), _dev(mask)
    with pytest.raises(RuntimeError):
        E.scene_metrics(torch.from_numpy(cano), t, ground, 'prox')                       # CPU tensor
    with pytest.raises(ValueError):
        E.scene_metrics(j, t, ground, 'kitti')
    with pytest.raises(ValueError):
        E.scene_metrics(j[:, :, :21], t, ground, 'prox')
    with pytest.raises(ValueError):
        E.scene_metrics(j, t[:1], ground, 'prox')
    with pytest.raises(ValueError):
        E.scene_metrics(j[:, :2], t, ground, 'prox')                                     # T < 3
    with pytest.raises(ValueError):
        E.scene_metrics(j, t, ground, 'egobody', g_[:, :15], k)                          # T_gt < T
    with pytest.raises(ValueError):
        E.scene_metrics(j, t, ground, 'egobody', g_, k[:, :15])
    with pytest.raises(ValueError):
        E.scene_metrics(j, t, ground, 'egobody')                                         # EgoBody needs GT + mask
    with pytest.raises(ValueError):
        E.scene_metrics(j, t, [0.0, 1.0, 2.0], 'prox')
    # the C ABI's own checks
    from rohm_amd._lib import RohmHipError, check, lib, ptr, stream_ptr
    out = torch.empty(2, 11, device=DEV, dtype=torch.float64)
    gh = torch.zeros(2, device=DEV)
    with pytest.raises(RohmHipError, match='up_axis'):
        check(lib().rohm_scene_metrics(ptr(j), ptr(t), ptr(gh), 0, None, 0, None, None, 2, 16, ptr(out), stream_ptr()), 'x')
    with pytest.raises(RohmHipError, match='T='):
        check(lib().rohm_scene_metrics(ptr(j), ptr(t), ptr(gh), 1, None, 0, None, None, 2, 801, ptr(out), stream_ptr()), 'x')
    with pytest.raises(RohmHipError, match='mask_vis'):
        check(lib().rohm_scene_metrics(ptr(j), ptr(t), ptr(gh), 1, None, 0, ptr(k), None, 2, 16, ptr(out), stream_ptr()), 'x')


def test_from_output_equals_joints_then_metrics():
    from rohm_amd.body_model import SMPLXLayer
    from rohm_amd.data_loaders.motion_representation import joints_from_repr
    from rohm_amd.utils import synth
    mean, std = synth.synthetic_stats(1)
    B, T = 3, 143
    x = synth.plausible_motion(5, B, T, mean, std).to(DEV)                    # [B, 294, 1, T] normalised
    layer = SMPLXLayer.from_tensors(synth.synthetic_smplx_tensors(0)).to(DEV)
    _, m, ground, gt, mask = _exact_clips(9, B, T, 'egobody')
    joints = joints_from_repr(x, 'smplx_params', layer, stats=(mean, std), layout='bc1t')
    ref = E.scene_metrics(joints, _dev(m), ground, 'egobody', _dev(gt), _dev(mask))
    got = E.scene_metrics_from_output(x, (mean, std), layer, _dev(m), ground, 'egobody', _dev(gt), _dev(mask))
    assert np.array_equal(got.sums, ref.sums)
    got = E.scene_metrics_from_output(x, (mean, std), layer, _dev(m), ground, 'prox')
    assert np.array_equal(got.sums[:, [0, 1, 3, 4]], E.scene_metrics(joints, _dev(m), ground, 'prox').sums[:, [0, 1, 3, 4]])


def _write_scene_pickles(g, dataset, family, d):
    heights = {}
    for r in R.golden_case(g, dataset, family):
        data = {'rec_ric_data_rec_list_from_smpl': r['joints_rec'], 'trans_scene2cano_list': r['trans_scene2cano'],
                'mask_joint_vis_list': r['mask'] if r['mask'] is not None else np.ones(r['joints_rec'].shape[:3], np.float32)}
        if dataset == 'egobody':
            data['joints_gt_scene_coord_list'] = r['joints_gt']
        with open(d / (r['name'] + '.pkl'), 'wb') as f:
            pickle.dump(data, f)
        heights[r['name']] = r['ground_height']
    return heights


@pytest.mark.parametrize('dataset', ['prox', 'egobody'])
def test_evaluator_main_prints_the_scripts_lines(dataset, tmp_path, capsys):
    import json
    g = golden('scene_metrics.npz')
    heights = _write_scene_pickles(g, dataset, 'exact', tmp_path)
    fh = tmp_path / 'floor.json'
    fh.write_text(json.dumps(heights))
    names = [r['name'] for r in R.golden_case(g, dataset, 'exact')]
    assert E.main(['--dataset', dataset, '--saved_data_dir', str(tmp_path), '--recordings', *names,
                   '--floor_heights', str(fh), '--json', str(tmp_path / 'out.json')]) == 0
    printed = capsys.readouterr().out
    assert printed == '\n'.join(g[f'{dataset}_exact_lines']) + '\n'
    numbers = json.loads((tmp_path / 'out.json').read_text())
    assert set(numbers['recordings']) == set(names)
    assert numbers['all']['skating'] == pytest.approx(float(g[f'{dataset}_exact_value_skating']), rel=1e-12)


def test_evaluator_main_amass(tmp_path, capsys):
    g = golden('scene_metrics.npz')
    clean, rec, r_clean, r_rec = M.synthetic_results(int(g['amass_results_seed']))
    data = {'repr_name_list': [], 'repr_dim_dict': {}, 'rec_ric_data_clean_list': clean,
            'rec_ric_data_rec_list_from_abs_traj': rec, 'rec_ric_data_rec_list_from_smpl': rec,
            'motion_repr_clean_list': r_clean, 'motion_repr_rec_list': r_rec}
    path = tmp_path / 'amass.pkl'
    with open(path, 'wb') as f:
        pickle.dump(data, f)
    assert E.main(['--dataset', 'amass', '--saved_data_path', str(path), '--mask_scheme', str(g['amass_mask_scheme'])]) == 0
    assert capsys.readouterr().out == '\n'.join(g['amass_lines']) + '\n'
