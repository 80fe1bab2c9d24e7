"""CPU: the host side of rohm_amd.drivers against tests/golden/drivers.npz (what the reference scripts' own text gives,
scripts/make_golden_drivers.py): argument tables, config files, pickle file names, the step schedule, ResultWriter, and the numpy
restatement of the trajectory report (tests/drivers_ref.py) that the GPU tests lean on."""
import glob
import json
import os
import pickle
import types

import numpy as np
import pytest
import torch

import drivers_ref as DR
from helpers import GOLDEN, golden
from rohm_amd.drivers import results as R
from rohm_amd.drivers.__main__ import OWN, SPECS, _bool, parse_args

TYPE_NAMES = {int: 'int', float: 'float', str: 'str', _bool: 'bool'}
CFG = sorted(glob.glob(os.path.join(GOLDEN, 'test_cfg', '*.yaml')))


@pytest.fixture(scope='module')
def gd():
    return golden('drivers.npz')


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize('which', list(SPECS))
def test_argument_tables_are_the_scripts(gd, which):
    ref = json.loads(str(gd['args_' + which]))
    assert [n for n, _, _ in SPECS[which]] == [r[0] for r in ref]
    for (name, default, typ), (_, rdefault, rtyp, _) in zip(SPECS[which], ref):
        assert TYPE_NAMES[typ] == rtyp, name
        assert default == rdefault and isinstance(default, {'int': int, 'float': float, 'str': str, 'bool': bool}[rtyp]), name
    a = parse_args(which, [])
    for name, rdefault, _, choices in ref:
        assert getattr(a, name) == rdefault, name
        if choices:
            with pytest.raises(SystemExit):
                parse_args(which, ['--' + name, 'no-such-choice'])
    assert not {n for n, _, _ in OWN[which]} & {r[0] for r in ref}


def test_booleans_follow_the_drivers_rule():
    a = parse_args('trajnet', ['--trajcontrol', 'True', '--infill_traj', '1', '--visualize', 'no', '--evaluate'])
    assert (a.trajcontrol, a.infill_traj, a.visualize, a.evaluate) == (True, True, False, True)
    assert parse_args('amass_full', ['--evaluate', 'false']).evaluate is False
    with pytest.raises(SystemExit):
        parse_args('amass_full', ['--visualize', 'True'])          # test_amass_full.py has no such argument


@pytest.mark.parametrize('path', CFG, ids=[os.path.basename(p) for p in CFG])
def test_shipped_configs_parse(path):
    which = 'amass_full' if os.path.basename(path).startswith('amass') else 'prox_egobody'
    a = parse_args(which, ['--config', path, '--seed', '3'])
    assert a.seed == 3 and a.clip_len == 145 and a.sample_iter == 2 and a.save_interval == 0 and a.evaluate is False
    if which == 'amass_full':
        assert a.mask_scheme == ('full' if 'occ_0.1' in path else 'lower') and a.load_noise is True
        assert a.load_noise_level == int(path.rsplit('_', 1)[1].split('.')[0])
    else:
        assert a.dataset == ('egobody' if 'egobody' in path else 'prox') and a.early_stop is True


def test_seven_configs_are_there():
    assert len(CFG) == 7


def test_an_unknown_setting_is_an_error(tmp_path):
    p = tmp_path / 'cfg.yaml'
    p.write_text("clip_len: 145\nno_such_setting: 1\n")
    with pytest.raises(ValueError, match='no_such_setting'):
        parse_args('amass_full', ['--config', str(p)])
    p.write_text("mask_scheme: sideways\n")
    with pytest.raises(ValueError, match='mask_scheme'):
        parse_args('amass_full', ['--config', str(p)])
    with pytest.raises(SystemExit):
        parse_args('posenet', ['--no_such_setting', '1'])


def test_pickle_file_names(gd):
    for row in gd['amass_full_file_names']:
        a, path = json.loads(str(row))
        assert R.amass_full_pickle_path(types.SimpleNamespace(**a)) == path
    for row in gd['prox_egobody_file_names']:
        a, rec, path = json.loads(str(row))
        assert R.prox_egobody_pickle_path(types.SimpleNamespace(**a), rec) == path
    for row in gd['posenet_file_names']:
        a, path = json.loads(str(row))
        assert R.posenet_pickle_path(types.SimpleNamespace(**a)) == path


def test_step_schedule():
    assert R.step_schedule(3, 2) == [0, 1]
    assert R.step_schedule(4, 2) == [0, 1, 0]          # a multiple of the batch size: the first batch a second time
    assert R.step_schedule(5, 2) == [0, 1, 2]
    assert R.step_schedule(0, 2) == []


def _static(gd, prefix):
    s = {'repr_name_list': [str(x) for x in gd['repr_name_list']],
         'repr_dim_dict': {str(k): int(v) for k, v in zip(gd['repr_name_list'], gd['repr_dim_list'])}}
    if prefix == 'amass_full':
        s['mask_scheme'] = str(gd['amass_full_save_mask_scheme'])
    if prefix in ('prox', 'egobody'):
        s['recording_name'] = str(gd[f'{prefix}_save_recording_name'])
    if prefix == 'egobody':
        s['gender_gt'] = str(gd['egobody_save_gender_gt'])
    return s


def _saved(gd, prefix, key):
    if prefix == 'egobody' and key != 'joints_gt_scene_coord_list':
        prefix = 'prox'          # the numeric entries are the same for both datasets and stored once
    return gd[f'{prefix}_save_{key}']


@pytest.mark.parametrize('prefix,keys', [('amass_full', R.AMASS_PICKLE_KEYS), ('posenet', R.POSENET_PICKLE_KEYS),
                                         ('prox', R.SCENE_PICKLE_KEYS), ('egobody', R.SCENE_PICKLE_KEYS)])
def test_result_writer_writes_the_scripts_pickle(gd, tmp_path, prefix, keys):
    ref_keys = [str(k) for k in gd[f'{prefix}_save_keys']]
    ref_types = [str(t) for t in gd[f'{prefix}_save_dtypes']]
    static = _static(gd, prefix)
    scene = prefix in ('prox', 'egobody')
    w = R.ResultWriter(str(tmp_path / 'sub' / 'out.pkl'), keys, static, last_only=('frame_name_list',) if scene else (),
                       save_interval=2)
    arrays = [k for k, t in zip(ref_keys, ref_types) if t == 'float32']
    a = 0
    for i, n in enumerate(DR.BATCHES):
        entries = {k: torch.from_numpy(_saved(gd, prefix, k)[a:a + n].copy()) for k in arrays}
        if scene:
            entries['frame_name_list'] = DR.prox_inputs(i, DR.stats(), prefix)['frame_name']
        w.add(entries)
        assert os.path.exists(w.path) == (i == 1)          # save_interval 2: written after the second batch
        a += n
    w.close()
    with open(w.path, 'rb') as f:
        raw = f.read()
    assert raw[:2] == b'\x80\x02'                            # protocol 2
    got = pickle.loads(raw)
    assert list(got.keys()) == ref_keys
    for k, t in zip(ref_keys, ref_types):
        if t == 'float32':
            ref = _saved(gd, prefix, k)
            assert got[k].dtype == np.float32 and got[k].shape == ref.shape and np.array_equal(bits(got[k]), bits(ref)), k
        elif k == 'frame_name_list':
            ref = gd[f'{prefix}_save_frame_name_list']
            assert isinstance(got[k], np.ndarray) and got[k].shape == ref.shape == (DR.BATCHES[-1], 17)      # the last batch only
            assert (got[k] == ref).all()
        else:
            assert type(got[k]).__name__ == t and got[k] == static[k], k
    with pytest.raises(KeyError):
        w.add({'no_such_key': torch.zeros(1)})


def test_posenet_contact_labels_of_earlier_batches_are_thresholded(gd):
    """test_posenet.py:260-265 writes 0 / 1 into the arrays its lists hold: the recorded file has thresholded contact labels for all
    batches but the last, and `threshold_contact_labels` reproduces that from the de-normalised values."""
    mean, std = DR.stats()
    n0 = DR.BATCHES[0]
    for key, name in (('motion_repr_rec_list', 'rec'), ('motion_repr_clean_list', 'clean')):
        saved = gd[f'posenet_save_{key}']
        assert set(np.unique(saved[:n0, :, -4:])) <= {0.0, 1.0} and not set(np.unique(saved[n0:, :, -4:])) <= {0.0, 1.0}
        raw = DR.denorm(DR.rows(DR.posenet_inputs(0, (mean, std))[name]).numpy(), mean, std)
        host = {'motion_repr_rec_list': raw.copy(), 'motion_repr_clean_list': raw.copy()}
        R.threshold_contact_labels(host)
        assert np.array_equal(bits(host[key]), bits(saved[:n0]))


def test_denorm_restatement_is_the_scripts(gd):
    st = DR.stats()
    a = 0
    for i, n in enumerate(DR.BATCHES):
        clean, rec, noisy = DR.amass_denorm(DR.amass_inputs(i, st), st)
        for got, key in ((clean, 'motion_repr_clean_list'), (rec, 'motion_repr_rec_list'), (noisy, 'motion_repr_noisy_list')):
            assert np.array_equal(bits(got), bits(gd['amass_full_save_' + key][a:a + n])), (i, key)
        a += n


@pytest.mark.parametrize('tag,T', [('t16', 16), ('t144', 144)])
def test_traj_report_restatement(gd, tag, T):
    joints = [np.concatenate([gd[f'trajnet_{tag}_b{i}_joints_{k}'] for i in range(2)]) for k in DR.JOINT_NAMES]
    rot = [np.concatenate([gd[f'trajnet_{tag}_b{i}_rot_{k}'] for i in range(2)]) for k in ('clean', 'rec')]
    err, jit, sums = DR.traj_report(joints, rot[0], rot[1])
    assert err.shape == (3, 10, T) and jit.shape == (3, 5, T - 3)
    assert np.array_equal(bits(err), bits(gd[f'trajnet_{tag}_elems_err']))          # bit for bit the script's per-element values
    assert np.array_equal(bits(jit), bits(gd[f'trajnet_{tag}_elems_jitter']))
    ref = gd[f'trajnet_{tag}_sums']
    assert np.abs(sums - ref).max() <= 1e-12 * np.abs(ref).max() and (np.abs(sums - ref) <= 1e-12 * np.abs(ref)).all()
    # TrajReport divides the same sums: its means agree with the script's float32 means to float32 accuracy
    rep = R.TrajReport(T, sums[:2]).merge(R.TrajReport(T, sums[2:]))
    assert rep.n_clips == 3
    means = gd[f'trajnet_{tag}_means']
    got = np.array(list(rep.summary().values()))
    assert list(rep.summary()) == DR.REPORT_ERR + DR.REPORT_JITTER
    assert np.abs(got - means).max() / np.abs(means).max() < 1e-5 and (np.abs(got - means) <= 2e-5 * np.abs(means)).all()
    with pytest.raises(ValueError):
        rep.merge(R.TrajReport(T + 1, sums))


@pytest.mark.parametrize('tag', ['t16', 't144'])
def test_traj_report_lines_from_the_scripts_means(gd, tag):
    means = gd[f'trajnet_{tag}_means']
    assert means.dtype == np.float32
    m = dict(zip(DR.REPORT_ERR + DR.REPORT_JITTER, means))
    assert R.traj_report_lines(m, 3) == [str(x) for x in gd[f'trajnet_{tag}_lines']]
