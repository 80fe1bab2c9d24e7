"""CPU: the host side of rohm_amd.preprocessing_amass -- which recordings are processed and at which down-sampling factor
(preprocessing_amass.py:23-40, :127-134), and the argument table against the script's own text where the reference is there."""
import ast
import os

import numpy as np
import pytest

from rohm_amd import preprocessing_amass as P

OK = ('neutral', 'smplx')

PLAN = [
    # dataset, recording, fps, gender, model type -> process, down_sample
    ('ACCAD', 'B1_-_stand_to_walk_stageii', 120.0, *OK, True, 4),
    ('CMU', '01_01_stageii', 60.0, *OK, True, 2),
    ('TotalCapture', 'acting1_stageii', 30.0, *OK, True, 1),
    ('KIT', 'bend_left01_stageii', 100.0, *OK, False, 3),
    ('Eyes_Japan_Dataset', 'accident-02-dodge_fast-aita_stageii', 250.0, *OK, False, 8),
    ('ACCAD', 'ntsc_stageii', 29.97, *OK, False, 0),
    ('SSM', 'punch_kick_sync_stageii', 59.9912, *OK, True, 2),
    ('SSM', 'resting_pose_stageii', 120.0031, *OK, True, 4),
    ('ACCAD', 'neutral_stagei', 120.0, *OK, False, 0),
    ('HDM05', 'HDM_dg_07-01_01_120_stageii', 120.0, *OK, False, 0),
    ('HDM05', 'HDM_dg_07-02_01_120_stageii', 120.0, *OK, True, 4),
    ('ACCAD', 'HDM_dg_07-01_01_120_stageii', 120.0, *OK, True, 4),          # the rule is HDM05's alone
    ('BMLrub', '0005_treadmill_norm_stageii', 120.0, *OK, False, 0),
    ('BMLrub', '0005_normal_walk1_stageii', 120.0, *OK, False, 0),
    ('BMLrub', '0005_jumping1_stageii', 120.0, *OK, True, 4),
    ('BMLmovi', '0005_treadmill_norm_stageii', 120.0, *OK, True, 4),        # ... and this one BMLrub's
    ('ACCAD', 'x_stageii', 120.0, 'female', 'smplx', False, 4),
    ('ACCAD', 'x_stageii', 120.0, 'neutral', 'smplh', False, 4),
    ('ACCAD', 'x_stageii', 120.0, b'neutral', 'smplx', False, 4),           # bytes != str, as in the script
]


@pytest.mark.parametrize('row', PLAN, ids=[f'{r[0]}-{r[1]}-{r[2]}-{r[3]!r}-{r[4]}' for r in PLAN])
def test_plan_recording(row):
    dataset, name, fps, gender, model, process, ds = row
    got = P.plan_recording(dataset, name, fps, gender, model)
    assert (got[0], got[1]) == (process, ds) and isinstance(got[0], bool) and isinstance(got[1], int)
    assert bool(got[2]) == (not process)                                    # a reason exactly where nothing is written
    # the values as np.load hands them over: 0-d arrays
    arr = P.plan_recording(dataset, name, np.array(fps), np.array(gender), np.array(model))
    assert arr[:2] == got[:2]


def test_reasons_name_what_the_script_prints():
    assert 'gender' in P.plan_recording('ACCAD', 'x', 120.0, 'male', 'smplx')[2]
    assert 'smplx' in P.plan_recording('ACCAD', 'x', 120.0, 'neutral', 'smplh')[2]
    assert 'frame rate 100.0' in P.plan_recording('ACCAD', 'x', 100.0, 'neutral', 'smplx')[2]
    both = P.plan_recording('ACCAD', 'x', 100.0, 'male', 'smplx')[2]
    assert 'gender' in both and 'frame rate' in both


def _write_raw(path, frames=7, fps=120.0, drop=()):
    g = np.random.Generator(np.random.PCG64(1))
    d = dict(mocap_frame_rate=np.array(fps), gender=np.array('neutral'), surface_model_type=np.array('smplx'),
             betas=g.standard_normal(16), trans=g.standard_normal((frames, 3)), root_orient=g.standard_normal((frames, 3)),
             pose_body=g.standard_normal((frames, 63)), pose_hand=g.standard_normal((frames, 90)),
             pose_jaw=g.standard_normal((frames, 3)), pose_eye=g.standard_normal((frames, 6)))
    for k in drop:
        del d[k]
    np.savez(path, **d)
    return d


def test_read_recording_keeps_every_ds_th_frame(tmp_path):
    path = str(tmp_path / 'a.npz')
    d = _write_raw(path, frames=11)
    r = P.read_recording('ACCAD', 'a', path)
    assert r['process'] and r['down_sample'] == 4 and r['frames'] == 3
    for k, n in P.FRAME_KEYS:
        assert r['arrays'][k].dtype == np.float64 and r['arrays'][k].shape == (3, n) and r['arrays'][k].flags.c_contiguous
        assert np.array_equal(r['arrays'][k], d[k][::4])
    assert np.array_equal(r['betas'], d['betas'][:10])


def test_read_recording_errors_name_the_file(tmp_path):
    path = str(tmp_path / 'broken.npz')
    _write_raw(path, drop=('pose_hand',))
    with pytest.raises(KeyError, match='broken.npz.*pose_hand'):
        P.read_recording('ACCAD', 'broken', path)
    _write_raw(path, drop=('gender',))
    with pytest.raises(KeyError, match='broken.npz.*gender'):
        P.read_recording('ACCAD', 'broken', path)
    _write_raw(path, frames=0)
    r = P.read_recording('ACCAD', 'broken', path)
    assert not r['process'] and r['reason'] == 'no frames'


def test_the_module_needs_no_hip_to_plan():
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; import rohm_amd.preprocessing_amass as P; P.plan_recording('ACCAD', 'x', 120.0, 'neutral', 'smplx'); "
            "assert 'rohm_amd._lib' not in sys.modules")
    r = subprocess.run([sys.executable, '-c', code], cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr


def test_own_arguments():
    assert [a[0] for a in P.OWN_ARGS] == ['device', 'chunk_frames', 'check_against', 'check_tol']
    a = P.build_parser().parse_args([])
    assert (a.device, a.chunk_frames, a.check_against, a.check_tol) == ('cuda:0', 262144, None, 1e-4)
    text = ' '.join(P.build_parser().format_help().split())
    assert 'smplx package' in text and 'pin' in text                        # the help says what this option can and cannot pin
    assert len(P.SCRIPT_ARGS) == 4 and P.READER_THREADS <= 8


def _script_arguments(path):
    """(name, type name, default) of every parser.add_argument call in the script's text."""
    rows = []
    for node in ast.walk(ast.parse(open(path).read())):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == 'add_argument':
            kw = {k.arg: k.value for k in node.keywords}
            rows.append((node.args[0].value.lstrip('-'), kw['type'].id, ast.literal_eval(kw['default'])))
    return rows


def test_argument_table_is_the_scripts():
    from oracle.refload import REF_ROOT
    script = os.path.join(REF_ROOT, 'preprocessing_amass.py')
    if not os.path.isfile(script):
        pytest.skip('the reference checkout is not here')
    ref = _script_arguments(script)
    assert [(n, t.__name__, d) for n, t, d, _ in P.SCRIPT_ARGS] == ref
    a = P.build_parser().parse_args([])
    for name, _, default in ref:
        assert getattr(a, name) == default and type(getattr(a, name)) is type(default)
    assert not {n for n, *_ in P.OWN_ARGS} & {r[0] for r in ref}
