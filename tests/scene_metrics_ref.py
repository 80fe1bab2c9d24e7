"""TEST INFRASTRUCTURE ONLY: numpy restatement of the PROX / EgoBody evaluation (eval_prox_egobody.py:172-270 per
recording, final block :453-490), pinned to the reference's own statements by tests/golden/scene_metrics.npz
(scripts/make_golden_scene_metrics.py).  `recording_arrays` returns the script's per-recording arrays, `final_lines`
what it prints, `clip_sums` the per-clip float64 sums `rohm_scene_metrics` produces (include/rohm_hip.h)."""
import numpy as np

FOOT = [7, 10, 8, 11]            # :189
FPS = 30
UP = {'prox': 2, 'egobody': 1}
HORIZ = {'prox': [0, 1], 'egobody': [0, 2]}
ARRAYS = ('skating', 'acc', 'acc_error', 'gmpjpe', 'mpjpe', 'mpjpe_vis', 'mpjpe_occ', 'pene_freq', 'pene_dist')


def points_coord_trans(xyz, m):
    """utils/other_utils.py:139-143."""
    return xyz.dot(m[:3, :3].transpose()) + m[:3, 3].reshape((1, -1))


def to_scene(joints_rec, trans_scene2cano):
    """:178-182: every clip back to scene coordinates (float32 in, float32 out)."""
    out = joints_rec.copy()
    n, T = out.shape[:2]
    for i in range(n):
        out[i] = points_coord_trans(out[i].reshape(-1, 3), np.linalg.inv(trans_scene2cano[i])).reshape(T, 22, 3)
    return out


def _elements(joints_rec, trans, ground_height, dataset, joints_gt=None, mask=None):
    rec = to_scene(joints_rec, trans)
    n, T = rec.shape[:2]
    up = UP[dataset]
    feet = rec[:, :, FOOT, :]
    vel = np.linalg.norm(feet[:, 1:][..., HORIZ[dataset]] - feet[:, :-1][..., HORIZ[dataset]], axis=-1) * FPS
    height = feet[:, 0:-1, :, up] - ground_height
    e = {'scene': rec, 'vel': vel, 'height': height}
    left = (vel[:, :, 0] > 0.10) * (vel[:, :, 1] > 0.10) * (height[:, :, 0] < (0.10 + 0.05)) * (height[:, :, 1] < 0.10)
    right = (vel[:, :, 2] > 0.10) * (vel[:, :, 3] > 0.10) * (height[:, :, 2] < (0.10 + 0.05)) * (height[:, :, 3] < 0.10)
    e['skating'] = left * right
    acc = (rec[:, 2:] - 2 * rec[:, 1:-1] + rec[:, :-2]) * (FPS ** 2)
    e['acc_el'] = np.linalg.norm(acc, axis=-1)
    if joints_gt is not None:
        gt = joints_gt[:, 0:T]
        acc_gt = (gt[:, 2:] - 2 * gt[:, 1:-1] + gt[:, :-2]) * (FPS ** 2)
        e['acc_error_el'] = np.linalg.norm(acc - acc_gt, axis=-1)
        e['gmpjpe'] = np.linalg.norm(gt - rec, axis=-1)
        e['mpjpe'] = np.linalg.norm((gt - gt[:, 0:T, [0]]) - (rec - rec[:, :, [0]]), axis=-1)
        if mask is not None:
            e['mpjpe_vis'] = e['mpjpe'] * mask
            e['mpjpe_occ'] = e['mpjpe'] * (1 - mask)
    e['pene'] = rec[:, :, [10, 11], up] - ground_height
    return e


def recording_arrays(joints_rec, trans, ground_height, dataset, joints_gt=None, mask=None):
    """The arrays the script appends per recording: skating [n, T-1], acc / acc_error [n, T-2], gmpjpe / mpjpe /
    mpjpe_vis / mpjpe_occ / mask [n, T, 22] (EgoBody), pene_freq / pene_dist [n, T]; plus the scene joints."""
    e = _elements(joints_rec, trans, ground_height, dataset, joints_gt, mask)
    out = {'joints_scene': e['scene'], 'skating': e['skating'], 'acc': e['acc_el'].mean(axis=-1)}
    if dataset == 'egobody':
        out['acc_error'] = e['acc_error_el'].mean(axis=-1)
        for k in ('gmpjpe', 'mpjpe', 'mpjpe_vis', 'mpjpe_occ'):
            out[k] = e[k]
        out['mask'] = mask
    pene = e['pene']
    out['pene_freq'] = (pene < -0.05).mean(axis=-1)
    pene = pene.copy()
    pene[pene >= 0] = 0
    out['pene_dist'] = pene.mean(axis=-1)
    return out


def final_lines(per_recording, dataset):
    """:453-490 on [recording_arrays(...) for each recording]: the printed lines (print's first argument)."""
    cat = lambda k: np.concatenate([r[k] for r in per_recording], axis=0)
    lines = ['\n --------------- evaluation metrics -------------',
             'skating score: {:0.3f}'.format(cat('skating').mean())]
    if dataset == 'prox':
        lines.append('||acc|| (m/s^2): {:0.2f}'.format(cat('acc').mean()))
    else:
        lines.append('acc errors (m/s^2): {:0.2f}'.format(cat('acc_error').mean()))
    lines.append('ground_pene_freq score (%): {:0.2f}'.format(cat('pene_freq').mean() * 100))
    lines.append('ground_pene_dist score (mm): {:0.2f}'.format(-cat('pene_dist').mean() * 1000))
    if dataset == 'egobody':
        mask = cat('mask')
        lines.append('-------------- gmpjpe/mpjpe/mpjpe-vis/mpjpe-occ (mm) --------------')
        lines.append('{:0.2f} / {:0.2f} / {:0.2f} / {:0.2f}'.format(
            cat('gmpjpe').mean() * 1000, cat('mpjpe').mean() * 1000, cat('mpjpe_vis').sum() / mask.sum() * 1000,
            cat('mpjpe_occ').sum() / (1 - mask).sum() * 1000))
    return lines


def final_numbers(per_recording, dataset):
    """The unrounded values behind `final_lines`, with SceneMetrics.summary()'s names."""
    cat = lambda k: np.concatenate([r[k] for r in per_recording], axis=0)
    out = {'skating': cat('skating').mean()}
    if dataset == 'prox':
        out['acc'] = cat('acc').mean()
    else:
        out['acc_error'] = cat('acc_error').mean()
    out['ground_pene_freq'] = cat('pene_freq').mean() * 100
    out['ground_pene_dist'] = -cat('pene_dist').mean() * 1000
    if dataset == 'egobody':
        mask = cat('mask')
        out['gmpjpe'] = cat('gmpjpe').mean() * 1000
        out['mpjpe'] = cat('mpjpe').mean() * 1000
        with np.errstate(divide='ignore', invalid='ignore'):
            out['mpjpe_vis'] = cat('mpjpe_vis').sum() / mask.sum() * 1000
            out['mpjpe_occ'] = cat('mpjpe_occ').sum() / (1 - mask).sum() * 1000
    return {k: float(v) for k, v in out.items()}


def clip_sums(joints_rec, trans, ground_height, dataset, joints_gt=None, mask=None):
    """[n, 11] float64 per-clip sums in rohm_scene_metrics' layout, from the script's own float32 elements."""
    e = _elements(joints_rec, trans, ground_height, dataset, joints_gt, mask)
    n = len(e['scene'])
    s = np.zeros((n, 11))
    f = lambda a: a.astype(np.float64).reshape(n, -1).sum(axis=1)
    s[:, 0] = f(e['skating'])
    s[:, 1] = f(e['acc_el'])
    pene = e['pene']
    s[:, 3] = f(pene < -0.05)
    s[:, 4] = f(np.where(pene >= 0, np.float32(0), pene))
    if joints_gt is not None:
        s[:, 2] = f(e['acc_error_el'])
        s[:, 5] = f(e['gmpjpe'])
        s[:, 6] = f(e['mpjpe'])
        if mask is not None:
            s[:, 7] = f(e['mpjpe_vis'])
            s[:, 8] = f(mask)
            s[:, 9] = f(e['mpjpe_occ'])
            s[:, 10] = f(1 - mask)
    return s


def near_threshold(joints_rec, trans, ground_height, dataset, tol=1e-5):
    """How many thresholded quantities lie within `tol` of their threshold (an ulp-level difference in the back-transform
    can flip them): (skating frames with any such entry, toe entries with d within tol of -0.05)."""
    e = _elements(joints_rec, trans, ground_height, dataset)
    hmax = np.array([0.10 + 0.05, 0.10, 0.10 + 0.05, 0.10], np.float32)
    near = (np.abs(e['vel'] - np.float32(0.10)) <= tol) | (np.abs(e['height'] - hmax) <= tol)
    return int(near.any(axis=-1).sum()), int((np.abs(e['pene'] - np.float32(-0.05)) <= tol).sum())


# ---- the fixture's compact encoding ----------------------------------------------------------------------------------
# Scene-coordinate joint tracks lie on a 2^-10 m grid, stored as a first frame and int8 steps along time: the GT, and the
# reconstruction as its difference from the GT's first T frames (a PROX run has no GT for the script; there the track
# only carries the data).  The canonical float32
# joints the driver would have pickled are derived from them and the float32 trans_scene2cano by `cano_from_scene`
# (float64 elementwise in a fixed order, one rounding), which is the same on every machine.  The script's [n, T, 22]
# arrays are stored as a sha256 of their float32 bytes plus per-clip sums (math.fsum: exact, order-free).

GRID = 2.0 ** -10
BIG = ('gmpjpe', 'mpjpe', 'mpjpe_vis', 'mpjpe_occ')


def encode_track(q):
    """int grid coordinates [n, T, 22, 3] -> (first frame int16 [n, 22, 3], int8 steps along T [n, T-1, 22, 3])."""
    q = np.asarray(q, np.int64)
    d = np.diff(q, axis=1)
    assert np.abs(q[:, 0]).max() < 2 ** 15 and np.abs(d).max() < 2 ** 7
    return q[:, 0].astype(np.int16), d.astype(np.int8)


def decode_track(first, steps):
    """-> scene coordinates in metres (float64, exact)."""
    q = np.concatenate([first[:, None].astype(np.int64), steps.astype(np.int64)], axis=1)
    return np.cumsum(q, axis=1).astype(np.float64) * GRID


def cano_from_scene(scene, trans_scene2cano):
    """float32 canonical joints x . R^T + t of float64 scene joints [n, T, 22, 3] and float32 matrices [n, 4, 4]."""
    m = trans_scene2cano.astype(np.float64)[:, None, None]
    out = np.empty(scene.shape, np.float32)
    for r in range(3):
        out[..., r] = ((scene[..., 0] * m[..., r, 0] + scene[..., 1] * m[..., r, 1]) + scene[..., 2] * m[..., r, 2]) \
            + m[..., r, 3]
    return out


def digest(a):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def clip_fsums(a):
    """[n, ...] -> [n] float64 exact sums per clip."""
    import math
    return np.array([math.fsum(np.asarray(clip, np.float64).reshape(-1)) for clip in a])


def encode_arrays(arrays, prefix):
    """The script's per-recording arrays -> npz entries."""
    out = {}
    for k, v in arrays.items():
        if k in BIG:
            out[prefix + k + '_sha256'] = np.str_(digest(v))
            out[prefix + k + '_clip_sums'] = clip_fsums(v)
        elif v.dtype == np.bool_:
            out[prefix + k + '_bits'] = np.packbits(v.reshape(-1))
            out[prefix + k + '_shape'] = np.array(v.shape)
        else:
            out[prefix + k] = v
    return out


def golden_case(g, dataset, family):
    """The recordings of one (dataset, transform family) case of tests/golden/scene_metrics.npz, as dicts of the
    driver pickle's arrays (joints_rec, trans_scene2cano, joints_gt, mask), name and ground_height, plus the script's
    per-recording arrays under 'ref' ([n, T, 22] ones as {'sha256', 'clip_sums'})."""
    key = f'{dataset}_{family}'
    out = []
    for ri in range(int(g[key + '_n_recordings'])):
        p = f'{key}_{ri}_'
        m = g[p + 'trans_scene2cano']
        r = {'name': str(g[p + 'name']), 'ground_height': float(g[p + 'ground_height']), 'trans_scene2cano': m,
             'joints_gt': None, 'mask': None}
        gt = decode_track(g[p + 'gt_first'], g[p + 'gt_steps'])
        rd = decode_track(g[p + 'rec_first'], g[p + 'rec_steps'])
        r['joints_rec'] = cano_from_scene(gt[:, :rd.shape[1]] + rd, m)
        if dataset == 'egobody':
            r['joints_gt'] = gt.astype(np.float32)
            shape = tuple(g[p + 'mask_shape'])
            r['mask'] = np.unpackbits(g[p + 'mask_bits'])[:int(np.prod(shape))].reshape(shape).astype(np.float32)
        ref = {}
        for k in ARRAYS:
            if k in BIG and p + k + '_sha256' in g.files:
                ref[k] = {'sha256': str(g[p + k + '_sha256']), 'clip_sums': g[p + k + '_clip_sums']}
            elif p + k + '_bits' in g.files:
                shape = tuple(g[p + k + '_shape'])
                ref[k] = np.unpackbits(g[p + k + '_bits'])[:int(np.prod(shape))].reshape(shape).astype(bool)
            elif p + k in g.files:
                ref[k] = g[p + k]
        r['ref'] = ref
        out.append(r)
    return out
