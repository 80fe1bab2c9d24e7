"""CPU: the numpy restatement of the PROX / EgoBody evaluation (tests/scene_metrics_ref.py) against the reference's own
statements (tests/golden/scene_metrics.npz), the per-clip sums behind SceneMetrics, the headless evaluator's floor-height
readers and its argument checks."""
import json
import math

import numpy as np
import pytest

import scene_metrics_ref as R
from helpers import golden
from rohm_amd import evaluation as E

CASES = [(d, f) for d in ('prox', 'egobody') for f in ('exact', 'general')]
CONT = ('acc', 'acc_error', 'gmpjpe', 'mpjpe', 'mpjpe_vis', 'mpjpe_occ', 'pene_dist')


def _restate(case, dataset):
    return [R.recording_arrays(r['joints_rec'], r['trans_scene2cano'], r['ground_height'], dataset, r['joints_gt'],
                               r['mask']) for r in case]


@pytest.mark.parametrize('dataset,family', CASES)
def test_restatement_reproduces_reference_arrays_and_lines(dataset, family):
    g = golden('scene_metrics.npz')
    case = R.golden_case(g, dataset, family)
    mine = _restate(case, dataset)
    for r, m in zip(case, mine):
        for k, ref in r['ref'].items():
            if isinstance(ref, dict):   # [n, T, 22] arrays: digest of the float32 bytes, exact per-clip sums
                if family == 'exact':
                    assert R.digest(m[k]) == ref['sha256'], k
                np.testing.assert_allclose(R.clip_fsums(m[k]), ref['clip_sums'], rtol=0 if family == 'exact' else 1e-6,
                                           err_msg=k)
            elif family == 'exact':     # the back-transform is exact: every array is bit-identical
                assert np.array_equal(m[k], ref), k
            elif k in CONT:             # the general family's back-transform goes through BLAS
                np.testing.assert_allclose(m[k], ref, rtol=1e-5, atol=1e-6, err_msg=k)
            else:
                assert np.abs(m[k].astype(np.float64) - ref).sum() <= sum(
                    R.near_threshold(r['joints_rec'], r['trans_scene2cano'], r['ground_height'], dataset)) * 2, k
    assert R.final_lines(mine, dataset) == list(g[f'{dataset}_{family}_lines'])


@pytest.mark.parametrize('dataset,family', CASES)
def test_clip_sums_give_the_scripts_numbers(dataset, family):
    """Per-clip float64 sums, merged over recordings and divided by counts (SceneMetrics.summary), give the script's
    float32 means to rel 1e-6 and print the same lines."""
    g = golden('scene_metrics.npz')
    case = R.golden_case(g, dataset, family)
    parts = [E.SceneMetrics(dataset, r['joints_rec'].shape[1],
                            R.clip_sums(r['joints_rec'], r['trans_scene2cano'], r['ground_height'], dataset, r['joints_gt'],
                                        r['mask'])) for r in case]
    sm = parts[0].merge(*parts[1:])
    for k, v in sm.summary().items():
        ref = float(g[f'{dataset}_{family}_value_{k}'])
        assert abs(v - ref) <= 1e-6 * abs(ref), (k, v, ref)
    assert sm.lines() == list(g[f'{dataset}_{family}_lines'])


def test_near_threshold_report():
    """How many thresholded entries of the general family sit within 1e-5 of their threshold (the slack the GPU test
    allows in the counts there)."""
    g = golden('scene_metrics.npz')
    for dataset in ('prox', 'egobody'):
        near = [R.near_threshold(r['joints_rec'], r['trans_scene2cano'], r['ground_height'], dataset)
                for r in R.golden_case(g, dataset, 'general')]
        print(dataset, 'general: near-threshold (skating frames, toe entries) per recording:', near)
        assert all(a >= 0 and b >= 0 for a, b in near)


def test_summary_empty_mask_is_nan_and_merge_checks():
    s = np.zeros((2, 11))
    s[:, 6] = s[:, 7] = 5.0
    s[:, 8] = 22 * 10
    sm = E.SceneMetrics('egobody', 10, s)
    out = sm.summary()
    assert math.isnan(out['mpjpe_occ']) and out['mpjpe_vis'] == pytest.approx(5.0 / 220 * 1000)
    assert 'acc' not in out and 'acc_error' in out
    assert set(E.SceneMetrics('prox', 10, s).summary()) == {'skating', 'acc', 'ground_pene_freq', 'ground_pene_dist'}
    assert sm.merge(sm).n_clips == 4 and sm.merge(sm).summary()['mpjpe'] == out['mpjpe']
    with pytest.raises(ValueError):
        sm.merge(E.SceneMetrics('egobody', 11, s))
    with pytest.raises(ValueError):
        sm.merge(E.SceneMetrics('prox', 10, s))
    with pytest.raises(ValueError):
        E.SceneMetrics('amass', 10, s)


def test_floor_height_readers(tmp_path):
    (tmp_path / 'utils').mkdir()
    (tmp_path / 'utils' / 'other_utils.py').write_text(
        'import cv2\nimport numpy as np\n\nLIMBS = [(0, 1)]\n'
        "prox_floor_height = {'SceneA': -0.5,\n                     'SceneB': -0.25}\n"
        "egobody_floor_height = {'room_1': -1.5, 'room_2': -0.75}\n\ndef f():\n    return cv2.x\n")
    (tmp_path / 'egobody_rohm_info.csv').write_text(
        'recording_name,target_start_frame,scene_name,view\nrec_a,0,room_2,master\nrec_b,3,room_1,sub_1\n')
    assert E.read_floor_heights(str(tmp_path), 'prox') == {'SceneA': -0.5, 'SceneB': -0.25}
    assert E.read_egobody_scenes(str(tmp_path)) == {'rec_a': 'room_2', 'rec_b': 'room_1'}
    assert E.recording_floor_heights('prox', ['SceneB_00001_01', 'SceneA_7_2'], rohm_root=str(tmp_path)) == \
        {'SceneB_00001_01': -0.25, 'SceneA_7_2': -0.5}
    assert E.recording_floor_heights('egobody', ['rec_b', 'rec_a'], rohm_root=str(tmp_path),
                                     dataset_root=str(tmp_path)) == {'rec_b': -1.5, 'rec_a': -0.75}
    js = tmp_path / 'floor.json'
    js.write_text(json.dumps({'rec_a': -1.25, 'rec_b': 0.5}))
    assert E.recording_floor_heights('egobody', ['rec_a'], floor_heights=str(js)) == {'rec_a': -1.25}
    with pytest.raises(KeyError):
        E.recording_floor_heights('egobody', ['rec_c'], floor_heights=str(js))
    with pytest.raises(ValueError):
        E.recording_floor_heights('egobody', ['rec_a'], rohm_root=str(tmp_path))       # no dataset_root for the csv
    with pytest.raises(ValueError):
        E.recording_floor_heights('prox', ['SceneA_1'])
    with pytest.raises(KeyError):
        E.read_floor_heights(str(tmp_path), 'amass')


def test_argument_errors_before_any_device_work(tmp_path):
    with pytest.raises(SystemExit):
        E.main(['--dataset', 'amass'])                              # no --saved_data_path
    with pytest.raises(SystemExit):
        E.main(['--dataset', 'prox'])                               # no --saved_data_dir
    with pytest.raises(SystemExit):
        E.main(['--dataset', 'egobody', '--saved_data_dir', str(tmp_path)])    # no pickles
    with pytest.raises(SystemExit):
        E.main(['--dataset', 'kitti', '--saved_data_dir', str(tmp_path)])
    with pytest.raises(ValueError):
        E.scene_metrics(None, None, 0.0, 'kitti')
    import torch
    with pytest.raises(RuntimeError):       # CPU tensors: no fallback
        E.scene_metrics(torch.zeros(1, 10, 22, 3), torch.eye(4)[None], 0.0, 'prox')


def test_evaluator_imports_no_viewer_or_renderer():
    import subprocess
    import sys
    code = ('import sys, rohm_amd.evaluation\n'
            "bad = [m for m in ('open3d', 'pyrender', 'cv2', 'smplx', 'pandas') if m in sys.modules]\n"
            'assert not bad, bad\n')
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, '-c', code], cwd=root, check=True)
