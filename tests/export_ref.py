"""TEST INFRASTRUCTURE ONLY: float64 numpy restatement of the export step (csrc/export.hip, include/rohm_hip.h
rohm_export_smplx): rows of the 294-channel representation -> per-frame SMPL-X parameters in scene or camera coordinates.

What the reference does in pieces (eval_prox_egobody.py:275-310): recover_from_repr_smpl 'smplx_params'
(data_loaders/motion_representation.py:373-388) turns the 6-D rotations into axis-angle; `np.linalg.inv(trans_scene2cano)`
takes vertices back to the scene.  Here the frame change is applied to the parameters, as update_globalRT_for_smplx does
with delta_T given (utils/other_utils.py:221-240).  Pinned to the reference's own functions by tests/golden/export.npz
(scripts/make_golden_export.py)."""
import numpy as np

PARAM_COLS = {'global_orient': (0, 3), 'transl': (3, 6), 'betas': (6, 16), 'body_pose': (16, 79)}
CH_ROT6D, CH_TRANS, CH_POSE6D, CH_BETAS, CH_CONTACT = 7, 16, 154, 280, 290


def rot6d_to_rotmat(x):
    """quaternion.py:482-501 in float64: x [..., 6] interleaved (a1x a2x a1y a2y a1z a2z) -> [..., 3, 3], columns b1 b2 b3."""
    x = np.asarray(x, np.float64).reshape(x.shape[:-1] + (3, 2))
    a1, a2 = x[..., 0], x[..., 1]
    b1 = a1 / np.maximum(np.sqrt((a1 * a1).sum(-1, keepdims=True)), 1e-12)
    u = a2 - (b1 * a2).sum(-1, keepdims=True) * b1
    b2 = u / np.maximum(np.sqrt((u * u).sum(-1, keepdims=True)), 1e-12)
    return np.stack([b1, b2, np.cross(b1, b2)], axis=-1)


def rotmat_to_rotvec(M):
    """[..., 3, 3] -> [..., 3]: the quaternion by its largest component (Markley), w >= 0, angle = 2 atan2(|v|, w) -- stable at
    angle 0 and at pi; |rotvec| <= pi.  The small-angle series keeps the factor finite."""
    M = np.asarray(M, np.float64)
    flat = M.reshape(-1, 3, 3)
    out = np.zeros((len(flat), 3))
    for n, m in enumerate(flat):
        dec = [m[0, 0], m[1, 1], m[2, 2], m[0, 0] + m[1, 1] + m[2, 2]]
        choice = 0
        for i in range(1, 4):
            if dec[i] > dec[choice]:
                choice = i
        q = np.zeros(4)                       # x, y, z, w
        if choice != 3:
            i = choice
            j, k = (i + 1) % 3, (i + 2) % 3
            q[i] = 1 - dec[3] + 2 * m[i, i]
            q[j] = m[j, i] + m[i, j]
            q[k] = m[k, i] + m[i, k]
            q[3] = m[k, j] - m[j, k]
        else:
            q[:] = [m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1], 1 + dec[3]]
        q = q / np.sqrt((q * q).sum())
        if q[3] < 0:
            q = -q
        ang = 2 * np.arctan2(np.sqrt((q[:3] * q[:3]).sum()), q[3])
        a2 = ang * ang
        sc = 2 + a2 / 12 + 7 * a2 * a2 / 2880 if ang <= 1e-3 else ang / np.sin(ang / 2)
        out[n] = sc * q[:3]
    return out.reshape(M.shape[:-2] + (3,))


def rodrigues(rv):
    """[..., 3] -> [..., 3, 3] (exact Rodrigues formula, float64)."""
    rv = np.asarray(rv, np.float64)
    ang = np.sqrt((rv * rv).sum(-1))[..., None, None]
    safe = np.where(ang > 0, ang, 1.0)
    k = rv / safe[..., 0]
    K = np.zeros(rv.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -k[..., 2], k[..., 1], k[..., 2]
    K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -k[..., 0], -k[..., 1], k[..., 0]
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)


def _six_d(R):
    """Rotation matrix -> the interleaved 6-D vector of its first two columns."""
    return np.stack([R[:, 0], R[:, 1]], axis=-1).reshape(6)


def hard_rotations():
    """Rows of 6-D vectors: the identity, angle 1e-7, angle pi - 1e-4, a non-unit non-orthogonal pair -> ([4, 6], angles)."""
    axis = np.array([0.6, -0.48, 0.64])
    rows = [_six_d(np.eye(3)), _six_d(rodrigues(axis * 1e-7)), _six_d(rodrigues(axis * (np.pi - 1e-4)))]
    skew = rodrigues(np.array([0.3, -0.8, 0.5]))
    rows.append(np.stack([2.5 * skew[:, 0], 0.4 * skew[:, 1] + 0.7 * skew[:, 0]], axis=-1).reshape(6))
    return np.stack(rows), axis


def fold_pelvis(body_tensors):
    """The rest-pose pelvis of the folded joint regressor as the library holds it: (Jt [3], Js [3, 10]) accumulated in
    float64 and stored in float32 (rohm_smplx_create)."""
    f = lambda v: np.asarray(v.detach().cpu() if hasattr(v, 'detach') else v, np.float32).astype(np.float64)
    jr, vt, sd = f(body_tensors['J_regressor'])[0], f(body_tensors['v_template']), f(body_tensors['shapedirs'])[:, :, :10]
    return (jr @ vt).astype(np.float32), np.einsum('v,vck->ck', jr, sd).astype(np.float32)


def denormalise(repr_rows, mean=None, std=None):
    """`x * std + mean` as two rounded float32 operations (numpy's, and rohm_result_rows')."""
    x = np.asarray(repr_rows, np.float32)
    if mean is None:
        return x
    return x * np.asarray(std, np.float32) + np.asarray(mean, np.float32)


def affine(transf=None, rigid=None):
    """A = rigid . inv(transf) [4, 4] float64; None is the identity."""
    A = np.eye(4) if transf is None else np.linalg.inv(np.asarray(transf, np.float64))
    return A if rigid is None else np.asarray(rigid, np.float64) @ A


def export_params(repr_clips, frame_clip, frame_t, pelvis, transf=None, rigid=None, mean=None, std=None):
    """repr_clips [C, T, 294] float32 -> (params [N, 79] float64, contact [N, 4] float32).  pelvis = fold_pelvis(...);
    transf [C, 4, 4] float32 or None; rigid [4, 4] or None.  An index outside [0, C) x [0, T) gives a NaN row."""
    repr_clips = np.asarray(repr_clips, np.float32)
    C, T = repr_clips.shape[:2]
    Jt, Js = (np.asarray(v, np.float32).astype(np.float64) for v in pelvis)
    N = len(frame_clip)
    params, contact = np.full((N, 79), np.nan), np.full((N, 4), np.nan, np.float32)
    for n in range(N):
        c, t = int(frame_clip[n]), int(frame_t[n])
        if not (0 <= c < C and 0 <= t < T):
            continue
        x32 = denormalise(repr_clips[c, t], mean, std)
        x = x32.astype(np.float64)
        A = affine(None if transf is None else transf[c], rigid)
        betas = x[CH_BETAS:CH_BETAS + 10]
        delta = Jt + Js @ betas
        R = rot6d_to_rotmat(x[CH_ROT6D:CH_ROT6D + 6])
        params[n, 0:3] = rotmat_to_rotvec(A[:3, :3] @ R)
        params[n, 3:6] = A[:3, :3] @ (x[CH_TRANS:CH_TRANS + 3] + delta) + A[:3, 3] - delta
        params[n, 6:16] = betas
        params[n, 16:79] = rotmat_to_rotvec(rot6d_to_rotmat(x[CH_POSE6D:CH_POSE6D + 126].reshape(21, 6))).reshape(63)
        contact[n] = x32[CH_CONTACT:CH_CONTACT + 4]
    return params, contact


def rot_component_mask(rv, lo=0.05, hi=np.pi - 0.1):
    """Rotation vectors whose angle lies in [lo, hi]: where a componentwise comparison is well conditioned."""
    ang = np.sqrt((np.asarray(rv, np.float64) ** 2).sum(-1))
    return (ang >= lo) & (ang <= hi)


def repeated_batch_rows(transf):
    """How many leading rows of the drivers' pickle are the first pass: the drivers' batch loop repeats its first batch when
    the loader runs out; the first r >= 1 whose trans_scene2cano equals row 0's bit for bit starts the repeat."""
    transf = np.asarray(transf)
    for r in range(1, len(transf)):
        if transf[r].tobytes() == transf[0].tobytes():
            return r
    return len(transf)


def world_params_of_tree(tree, dataset, body_tensors):
    """World-frame SMPL-X rows [N, 79] (float64) of a synthetic tree (tests/video_tree.py): what the reference's loader
    holds after its per-frame update_globalRT_for_smplx (oracle.frames.frames_to_world)."""
    from oracle import frames as OF
    from oracle import geometry as G
    import video_tree as VT
    prm = {k: np.asarray(tree['params'][:, a:b], np.float32) for k, (a, b) in VT.PARAM_SLICES.items()}
    cam2world = tree['cam2world'] if dataset == 'prox' else tree['master2world'] @ tree['sub2main']
    return OF.frames_to_world(G.BodyModel(body_tensors), prm, np.asarray(cam2world, np.float32))[1], cam2world


def param_errors(got, want):
    """(largest rotation-matrix difference over the 22 rotations, largest translation difference, largest betas difference)."""
    rv = lambda p: np.concatenate([p[:, 0:3].reshape(-1, 1, 3), p[:, 16:79].reshape(-1, 21, 3)], axis=1)
    return (float(np.abs(rodrigues(rv(got)) - rodrigues(rv(want))).max()), float(np.abs(got[:, 3:6] - want[:, 3:6]).max()),
            float(np.abs(got[:, 6:16] - want[:, 6:16]).max()))


_ROUNDTRIP = {}


def roundtrip_cpu(golden_video_loader, body_tensors, plan):
    """The restatement on the clips the REFERENCE's loader made of the synthetic trees (tests/golden/video_loader.npz:
    `motion_repr_noisy`, `transf_matrix` of the 'pose' task) against the trees' world-frame parameters -> {dataset: (rotation
    matrix error, translation error)} and the largest of all: `roundtrip_cpu_error`, the distance the float32
    representation itself puts between the two."""
    if not _ROUNDTRIP:
        import video_tree as VT
        g = golden_video_loader
        pelvis = fold_pelvis(body_tensors)
        for dataset in ('prox', 'egobody'):
            tree = VT.tree_arrays_from_fixture(g, dataset)
            world, _ = world_params_of_tree(tree, dataset, body_tensors)
            rep = np.stack([g[f'{dataset}_pose_min_item{i}_motion_repr_noisy'] for i in range(3)]).astype(np.float32)
            tf = np.stack([g[f'{dataset}_pose_min_item{i}_transf_matrix'] for i in range(3)]).astype(np.float32)
            fc, ft, n = plan(3, rep.shape[1], VT.CLIP_LEN, VT.OVERLAP)
            got, _ = export_params(rep, fc, ft, pelvis, transf=tf, mean=tree['mean'], std=tree['std'])
            _ROUNDTRIP[dataset] = param_errors(got, world[:n])
        _ROUNDTRIP['roundtrip_cpu_error'] = max(max(v[:2]) for v in _ROUNDTRIP.values())
    return _ROUNDTRIP
