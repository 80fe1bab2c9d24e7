"""Golden vectors of the test drivers' result tails -> tests/golden/drivers.npz and tests/golden/test_cfg/*.yaml.

The method of oracle/make_golden.py::golden_scheme_real: the reference scripts' OWN TEXT, by line range, is compiled and executed
on the CPU in a prepared namespace (synthetic batches and sampler outputs, the oracle's body model standing for `smplx`, the
reference's own recover_from_repr_smpl); nothing of it is copied here.  Executed:
  test_amass_full.py     :194-200 (the lists), :387-455 (the tail), :456-463 (the file name)
  test_prox_egobody.py   :174-182, :327-384, :386-390
  test_posenet.py        :125-131, :185-252, :253-254, and :260-265 after each batch (see below)
  test_trajnet.py        :118-129, :160-264, :332-366
Every tail runs on TWO batches, of 2 clips and of 1 clip, so `save_data` holds three clips and a batch's entries are its rows.  Clips
are 16 / 15 frames (clip_len 17); the trajectory report also runs at 144 frames (pelvis tracks stored only), and the
de-normalisation at B = 3, T = 143 (results as sha256 of their bytes).  The inputs are seeded (tests/drivers_ref.py builds them
for this script and for the tests alike), so the fixture stores results only.  test_posenet.py:260-265 thresholds the
contact channels of `motion_repr_rec` / `motion_repr_clean` IN PLACE after a batch has been saved; the arrays are the ones held
in the lists, so every later save (and the final file) holds thresholded contact labels for all batches but the last.  The
recorded `save_data` has that.
Also stored: the scripts' argument names, defaults and types, read with `ast` (no import); the file names their format
expressions give for two argument sets each; the trajectory report's per-element values, per-clip float64 sums and printed
lines.  The seven cfg_files/test_cfg/*.yaml hold only settings and are copied.
Needs a RoHM checkout at oracle.refload.REF_ROOT; run once where it exists (CPU), commit only the fixtures:
    python scripts/make_golden_drivers.py
"""
import ast
import hashlib
import json
import os
import shutil
import sys
import textwrap
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refload  # noqa: E402
from rohm_amd.utils import synth  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import drivers_ref as DR  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
SCRIPTS = {'amass_full': 'test_amass_full.py', 'prox_egobody': 'test_prox_egobody.py', 'posenet': 'test_posenet.py',
           'trajnet': 'test_trajnet.py'}
STATS_SEED, BODY_SEED = 0, 0
ARRAY_KEYS = {
    'amass_full': ['rec_ric_data_clean_list', 'rec_ric_data_noisy_list', 'rec_ric_data_rec_list_from_abs_traj',
                   'rec_ric_data_rec_list_from_smpl', 'motion_repr_clean_list', 'motion_repr_noisy_list', 'motion_repr_rec_list'],
    'posenet': ['rec_ric_data_clean_list', 'rec_ric_data_noisy_list', 'rec_ric_data_rec_list_from_abs_traj',
                'rec_ric_data_rec_list_from_smpl', 'motion_repr_clean_list', 'motion_repr_noisy_list', 'motion_repr_rec_list'],
    'prox_egobody': ['joints_gt_scene_coord_list', 'trans_scene2cano_list', 'rec_ric_data_noisy_list',
                     'rec_ric_data_rec_list_from_abs_traj', 'rec_ric_data_rec_list_from_smpl', 'joints_input_scene_coord_list',
                     'motion_repr_noisy_list', 'motion_repr_rec_list', 'mask_joint_vis_list'],
}


def lines_of(which):
    with open(os.path.join(refload.REF_ROOT, SCRIPTS[which])) as f:
        return f.read().split('\n')


def block(which, first, last):
    """Lines first..last (1-based, inclusive) of a script, dedented and compiled."""
    text = textwrap.dedent('\n'.join(lines_of(which)[first - 1:last]))
    return compile(text, f'{SCRIPTS[which]}[{first}:{last}]', 'exec')


def argument_table(which):
    """[[name, default, type], ...] of the script's add_argument calls, read with ast: type is 'int' | 'float' | 'str' | 'bool'
    (the scripts' `lambda x: x.lower() in ['true', '1']`); a string default goes through the type as argparse does."""
    with open(os.path.join(refload.REF_ROOT, SCRIPTS[which])) as f:
        tree = ast.parse(f.read())
    rows = []
    for node in ast.walk(tree):
        if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == 'add_argument'):
            continue
        name = ast.literal_eval(node.args[0]).lstrip('-')
        kw = {k.arg: k.value for k in node.keywords}
        if name == 'config':
            continue
        typ = 'bool' if isinstance(kw['type'], ast.Lambda) else kw['type'].id
        default = ast.literal_eval(kw['default'])
        if isinstance(default, str) and typ != 'str':
            default = default.lower() in ['true', '1'] if typ == 'bool' else {'int': int, 'float': float}[typ](default)
        choices = ast.literal_eval(kw['choices']) if 'choices' in kw else None
        rows.append([name, default, typ, choices, node.lineno])
    rows.sort(key=lambda r: r[-1])
    return [r[:-1] for r in rows]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def base_namespace(ref, body, args):
    fake_os = types.SimpleNamespace(makedirs=lambda *a, **k: None,
                                    path=types.SimpleNamespace(exists=lambda p: True, join=os.path.join))
    return {'np': np, 'torch': torch, 'os': fake_os, 'args': args, 'print': lambda *a, **k: None,
            'dist_util': types.SimpleNamespace(dev=lambda: torch.device('cpu')), 'smplx_neutral': body,
            'REPR_LIST': ref.other_utils.REPR_LIST, 'REPR_DIM_DICT': ref.other_utils.REPR_DIM_DICT,
            'recover_from_repr_smpl': ref.motion_repr.recover_from_repr_smpl}


def dataset(stats, **kw):
    return types.SimpleNamespace(Mean=stats[0], Std=stats[1], traj_feat_dim=22, **kw)


def save_entries(out, prefix, save_data, keys):
    for k in keys:
        if k in save_data:
            out[f'{prefix}_save_{k}'] = np.asarray(save_data[k])
    out[f'{prefix}_save_keys'] = np.array(list(save_data.keys()))
    out[f'{prefix}_save_dtypes'] = np.array([str(np.asarray(save_data[k]).dtype) if isinstance(save_data[k], np.ndarray)
                                             else type(save_data[k]).__name__ for k in save_data])


def golden_amass_full(ref, body, stats, out):
    args = types.SimpleNamespace(input_noise=True, mask_scheme='lower', save_root='r')
    ns = base_namespace(ref, body, args)
    ns['test_pose_dataset'] = dataset(stats)
    exec(block('amass_full', 194, 200), ns)
    for i in range(2):
        inp = DR.amass_inputs(i, stats)
        ns.update(test_batch_pose={'motion_repr_clean': inp['clean'].clone(), 'motion_repr_noisy': inp['noisy'].clone()},
                  val_output_pose=inp['rec'].clone(), traj_noisy_full=inp['traj_noisy_full'].numpy().copy())
        exec(block('amass_full', 387, 455), ns)
    save_entries(out, 'amass_full', ns['save_data'], ARRAY_KEYS['amass_full'])
    out['amass_full_save_mask_scheme'] = ns['save_data']['mask_scheme']
    out['repr_name_list'] = np.array(ns['save_data']['repr_name_list'])
    out['repr_dim_list'] = np.array([ns['save_data']['repr_dim_dict'][k] for k in ns['save_data']['repr_name_list']])
    names = []
    for a in (dict(cond_fn_with_grad=True, mask_scheme='lower', input_noise=True, load_noise=True, load_noise_level=3,
                   infill_traj=False, traj_mask_ratio=0.1, sample_iter=2, iter2_cond_noisy_traj=True, iter2_cond_noisy_pose=True,
                   early_stop=False, seed=0, save_root='test_results/results_amass_full'),
              dict(cond_fn_with_grad=False, mask_scheme='full', input_noise=True, load_noise=False, load_noise_level=5,
                   infill_traj=True, traj_mask_ratio=0.1, sample_iter=3, iter2_cond_noisy_traj=False, iter2_cond_noisy_pose=True,
                   early_stop=True, seed=7, save_root='out')):
        ns2 = {'os': os, 'args': types.SimpleNamespace(**a)}
        exec(block('amass_full', 456, 463), ns2)
        names.append(json.dumps([a, ns2['pkl_path']]))
    out['amass_full_file_names'] = np.array(names)


def golden_rows_large(ref, body, stats, out):
    """test_amass_full.py:387-396 alone (the de-normalisation) at B = 3, T = 143: sha256 of the three arrays, and of the noisy
    one without the trajectory override (test_posenet.py:188-193)."""
    inp = DR.rows_large_inputs(stats)
    T = inp['clean'].shape[-1]
    ns = base_namespace(ref, body, types.SimpleNamespace(input_noise=True))
    ns['test_pose_dataset'] = dataset(stats)
    ns.update(test_batch_pose={'motion_repr_clean': inp['clean'].clone(), 'motion_repr_noisy': inp['noisy'][:, 0:T].clone()},
              val_output_pose=inp['rec'].clone(), traj_noisy_full=inp['traj_noisy_full'].numpy().copy())
    exec(block('amass_full', 387, 396), ns)
    got = [ns['motion_repr_clean'], ns['motion_repr_rec'], ns['motion_repr_noisy']]
    plain = inp['noisy'][:, 0:T].numpy() * stats[1] + stats[0]
    assert all(g.dtype == np.float32 and g.shape == (3, T, 294) for g in got + [plain])
    for g, r in zip(got, DR.amass_denorm(inp, stats, T)):
        assert np.array_equal(g.view(np.uint32), r.view(np.uint32))
    out['rows_large_sha'] = np.array([sha(g) for g in got + [plain]])


def golden_posenet(ref, body, stats, out):
    args = types.SimpleNamespace(input_noise=True, save_results=True)
    ns = base_namespace(ref, body, args)
    ns['test_dataset'] = dataset(stats)
    exec(block('posenet', 125, 131), ns)
    for i in range(2):
        inp = DR.posenet_inputs(i, stats)
        ns.update(test_batch={'motion_repr_clean': inp['clean'].clone(), 'motion_repr_noisy': inp['noisy'].clone()},
                  val_output=inp['rec'].clone())
        exec(block('posenet', 185, 252), ns)
        exec(block('posenet', 260, 265), ns)
    save_entries(out, 'posenet', ns['save_data'], ARRAY_KEYS['posenet'])
    names = []
    for a in (dict(model_path='checkpoints/posenet_checkpoint/model000200000.pt', cond_fn_with_grad=False),
              dict(model_path='runs/12345/model000025000.pt', cond_fn_with_grad=True)):
        ns2 = {'os': os, 'args': types.SimpleNamespace(**a), 'log_dir': '/'.join(a['model_path'].split('/')[0:-1])}
        exec(block('posenet', 253, 254), ns2)
        names.append(json.dumps([a, ns2['pkl_path']]))
    out['posenet_file_names'] = np.array(names)


def golden_prox_egobody(ref, body, stats, out):
    saved = {}
    for ds_name in ('prox', 'egobody'):
        args = types.SimpleNamespace(dataset=ds_name, save_root='r', cond_fn_with_grad=True, sample_iter=2,
                                     iter2_cond_noisy_traj=False, iter2_cond_noisy_pose=False, early_stop=True, seed=0)
        ns = base_namespace(ref, body, args)
        ns['test_pose_dataset'] = dataset(stats, gender_gt='female', recording_name='rec_' + ds_name)
        exec(block('prox_egobody', 174, 182), ns)
        for i in range(2):
            inp = DR.prox_inputs(i, stats, ds_name)
            tensors = {k: v.clone() for k, v in inp.items() if k not in ('noisy', 'rec', 'frame_name')}
            ns.update(test_batch_pose=dict(motion_repr_noisy=inp['noisy'].clone(), frame_name=inp['frame_name'], **tensors),
                      val_output_joint=inp['rec'].clone(), mask_joint_vis=tensors['mask_joint_vis'][:, 0:-2, :])     # :307
            exec(block('prox_egobody', 327, 384), ns)
        saved[ds_name] = sd = ns['save_data']
        out[f'{ds_name}_save_frame_name_list'] = np.asarray(sd['frame_name_list'])
        out[f'{ds_name}_save_recording_name'] = sd['recording_name']
    # the numeric entries do not depend on the dataset: stored once (PROX's), EgoBody's two extra entries next to them
    for k in ARRAY_KEYS['prox_egobody']:
        if k in saved['prox']:
            assert np.array_equal(saved['prox'][k], saved['egobody'][k])
    save_entries(out, 'prox', saved['prox'], ARRAY_KEYS['prox_egobody'])
    save_entries(out, 'egobody', saved['egobody'], ['joints_gt_scene_coord_list'])
    out['egobody_save_gender_gt'] = saved['egobody']['gender_gt']
    names = []
    for a in (dict(dataset='prox', cond_fn_with_grad=True, sample_iter=2, iter2_cond_noisy_traj=False, iter2_cond_noisy_pose=False,
                   early_stop=True, seed=0, save_root='test_results/results_prox_rgb'),
              dict(dataset='egobody', cond_fn_with_grad=False, sample_iter=1, iter2_cond_noisy_traj=True, iter2_cond_noisy_pose=True,
                   early_stop=False, seed=3, save_root='out')):
        rec_name = 'N0Sofa_00034_02' if a['dataset'] == 'prox' else 'recording_20210907_S02_S01_01'
        fake_os = types.SimpleNamespace(makedirs=lambda *x, **k: None, path=types.SimpleNamespace(exists=lambda p: True, join=os.path.join))
        ns2 = {'os': fake_os, 'args': types.SimpleNamespace(**a), 'test_pose_dataset': types.SimpleNamespace(recording_name=rec_name)}
        exec(block('prox_egobody', 386, 390), ns2)
        names.append(json.dumps([a, rec_name, ns2['pkl_path']]))
    out['prox_egobody_file_names'] = np.array(names)


def golden_trajnet(ref, body, stats, out):
    body_t = synth.synthetic_smplx_tensors(BODY_SEED)
    for tag, T, full in (('t16', 16, True), ('t144', 144, False)):
        args = types.SimpleNamespace(repr_abs_only=True, visualize=False, infill_traj=False)
        ns = base_namespace(ref, body, args)
        printed = []
        ns['print'] = lambda *a, **k: printed.append(' '.join(str(x) for x in a))
        ns['test_dataset'] = dataset(stats)
        ns['traj_feat_dim'] = 13
        exec(block('trajnet', 118, 129), ns)
        for i in range(2):
            inp = DR.trajnet_inputs(i, stats, T, body_t)
            ns.update(test_batch={'motion_repr_clean': inp['clean'].clone(), 'motion_repr_noisy': inp['noisy'].clone()},
                      val_output=inp['val_output'].clone())
            exec(block('trajnet', 160, 264), ns)
            pre = f'trajnet_{tag}_b{i}_'
            out[pre + 'rot_clean'] = ns['motion_repr_clean'][:, :, 0].copy()
            out[pre + 'rot_rec'] = ns['motion_repr_clean_root_rec'][:, :, 0].copy()
            for name in DR.JOINT_NAMES:
                j = ns['rec_ric_data_' + name]
                out[pre + 'joints_' + name] = j.copy() if full else j[:, :, 0:1].copy()
            if full and i == 0:
                out[pre + 'repr_clean'] = ns['motion_repr_clean'].copy()
                out[pre + 'repr_root_noisy'] = ns['motion_repr_clean_root_noisy'].copy()
                out[pre + 'repr_root_rec'] = ns['motion_repr_clean_root_rec'].copy()
        lists = [k + '_list' for k in DR.REPORT_ERR + DR.REPORT_JITTER]
        elems = [np.stack(ns[k]) for k in lists]                                             # 10 x [n, T], 5 x [n, T - 3]
        assert all(e.dtype == np.float32 for e in elems)
        out[f'trajnet_{tag}_elems_err'] = np.stack(elems[:10], axis=1)                       # [n, 10, T]
        out[f'trajnet_{tag}_elems_jitter'] = np.stack(elems[10:], axis=1)                    # [n, 5, T - 3]
        out[f'trajnet_{tag}_sums'] = np.stack([e.astype(np.float64).sum(axis=1) for e in elems], axis=1)      # [n, 15]
        # the float32 means the script formats (numpy's .mean() of the concatenated lists; Python's sum() / len() for the jitter)
        out[f'trajnet_{tag}_means'] = np.array([np.concatenate(list(e)).mean() for e in elems[:10]] +
                                               [sum(np.concatenate(list(e))) / e.size for e in elems[10:]], dtype=np.float32)
        exec(block('trajnet', 332, 366), ns)
        out[f'trajnet_{tag}_lines'] = np.array(printed)
        print(tag, printed)


def main():
    ref = refload.load()
    from oracle import geometry as G
    body = G.BodyModel(synth.synthetic_smplx_tensors(BODY_SEED))
    refload.set_body_model(body)
    stats = synth.synthetic_stats(STATS_SEED)
    out = {'stats_seed': STATS_SEED, 'body_seed': BODY_SEED}
    for which in SCRIPTS:
        out['args_' + which] = json.dumps(argument_table(which))
    golden_amass_full(ref, body, stats, out)
    golden_rows_large(ref, body, stats, out)
    golden_posenet(ref, body, stats, out)
    golden_prox_egobody(ref, body, stats, out)
    golden_trajnet(ref, body, stats, out)
    path = os.path.join(GOLD, 'drivers.npz')
    np.savez_compressed(path, **out)
    print('drivers.npz', os.path.getsize(path), 'bytes,', len(out), 'entries')
    dst = os.path.join(GOLD, 'test_cfg')
    os.makedirs(dst, exist_ok=True)
    src = os.path.join(refload.REF_ROOT, 'cfg_files', 'test_cfg')
    for f in sorted(os.listdir(src)):
        if f.endswith('.yaml'):
            shutil.copyfile(os.path.join(src, f), os.path.join(dst, f))


if __name__ == '__main__':
    main()
