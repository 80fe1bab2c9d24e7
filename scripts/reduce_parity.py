"""The record profiles/reduce_parity.json: every entry point over csrc/reduce.h once with the parent commit's library and once with this
tree's, on identical inputs at the shapes where the helpers can go wrong, all outputs compared as integers.

    git archive HEAD~1 rohm_amd/csrc include | tar -x -C /tmp/prev && python scripts/build_variant.py parent --src /tmp/prev/rohm_amd/csrc
    ROHM_HIP_LIB=$PWD/rohm_amd/librohm_hip_parent.so python scripts/reduce_parity.py run /tmp/parent.npz
    python scripts/reduce_parity.py run /tmp/new.npz
    python scripts/reduce_parity.py cmp /tmp/parent.npz /tmp/new.npz profiles/reduce_parity.json

The inputs come from tests/rig_ref.py's scenes and seeded generators; the shapes are point counts of 1, 63, 64, 65, 255, 257 and 1025, K
hypotheses of 1, a block's worth -+ 1 and all degenerate, V = 2 and 16, and quality tracks with a NaN row in each group."""
import json
import os
import sys

import numpy as np


def run(path):
    import torch


    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))

    import fit_ref as FR  # noqa: E402
    import rig_ref as RR  # noqa: E402
    from rohm_amd import _lib, floor, multiview, quality, rig, sync  # noqa: E402
    from rohm_amd._lib import check, lib, ptr, stream_ptr  # noqa: E402
    from rohm_amd.fit import shape_moments  # noqa: E402
    from rohm_amd.utils import synth  # noqa: E402

    DEV = 'cuda:0'
    POINTS = (1, 63, 64, 65, 255, 257, 1025)
    OUT = {}


    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


    def keep(name, *tensors):
        torch.cuda.synchronize()
        for i, t in enumerate(tensors):
            OUT[f'{name}#{i}'] = t.detach().cpu().numpy()


    def rng(seed):
        return np.random.Generator(np.random.PCG64(seed))


    # ---- floor ----
    for P in POINTS:
        g = rng(100 + P)
        pts = np.concatenate([g.uniform(-2, 2, (P, 2)), g.normal(0, 0.02, (P, 1))], 1).astype(np.float32)
        pts[::7, 2] += 0.5
        plane = np.array([0.01, -0.02, 1.0, 0.003]); plane[:3] /= np.linalg.norm(plane[:3])
        keep(f'floor_moments P={P}', floor.floor_moments(dev(pts), dev(plane), dev(pts.mean(0).astype(np.float64)), tau=0.03))
        if P >= 3:
            jts = np.concatenate([g.uniform(-2, 2, (P + 5, 2)), g.uniform(-0.2, 1.7, (P + 5, 1))], 1).astype(np.float32)
            for K in (1, 15, 17, 1023, 1025):
                tr = floor.draw_triples(P, K, 7 + K)
                keep(f'floor_hypotheses P={P} K={K}', *floor.floor_hypotheses(dev(pts), dev(jts), dev(tr)))
            tr = np.repeat(np.arange(17, dtype=np.int32)[:, None] % P, 3, 1)      # every triple one point three times: all degenerate
            keep(f'floor_hypotheses P={P} K=17 all degenerate', *floor.floor_hypotheses(dev(pts), dev(jts), dev(tr)))

    # ---- rig, sync, multiview ----
    for V in (2, 16):
        Kc, W, D, kp, X = RR.make_scene(V, 48, 22, 5 + V, noise_px=2.0, outlier_share=0.1)
        cams = multiview.pack_cameras(Kc, W, D)
        kp_flat, X_flat = kp.reshape(V, 48 * 22, 1, 3), X.reshape(48 * 22, 3)
        pairs = np.array([(a, b) for a in range(V) for b in range(a + 1, V)][:6] + [(0, 0)], dtype=np.int32)      # the last pair is refused by the kernel
        Q = len(pairs)
        E_true = np.stack([sync.essential(W, int(a), int(b)) if a != b else np.zeros(9) for a, b in pairs])
        for P in POINTS:
            k, Xp = dev(kp_flat[:, :P]), X_flat[:P]
            g = rng(1000 * V + P)
            for K in (1, 31, 33) + ((255, 257) if P in (65, 1025) else ()):      # a scoring block's worth, the arg-max block's worth, -+ 1
                sm = g.integers(0, P, (Q, K, 8)).astype(np.int32)
                keep(f'rig_pair_hypotheses V={V} P={P} K={K}', *rig.pair_hypotheses(k, dev(cams), dev(pairs), dev(sm), tau_px=4.0))
            sm = np.zeros((Q, 33, 8), np.int32)                                  # repeated indices: all degenerate
            keep(f'rig_pair_hypotheses V={V} P={P} K=33 all degenerate', *rig.pair_hypotheses(k, dev(cams), dev(pairs), dev(sm), tau_px=4.0))
            keep(f'rig_pair_moments V={V} P={P}', rig.pair_moments(k, dev(cams), dev(pairs), dev(E_true), tau_px=4.0))
            pts = Xp + g.normal(0, 0.01, Xp.shape)
            keep(f'rig_ba_moments V={V} P={P}', *rig.ba_moments(k, dev(cams), dev(pts)))
            keep(f'rig_ba_update V={V} P={P}', *rig.ba_update(k, dev(cams), dev(pts), dev(g.normal(0, 1e-3, (V, 6)))))
            sh = np.array([[0.0, 1.0, -2.0, 0.37, -1.62, 3.5]] * Q)
            keep(f'sync_pair_sweep V={V} N={P} J=1', sync.pair_sweep(k, dev(cams), dev(pairs), dev(E_true), dev(sh)))
            tri = multiview.triangulate(k, dev(cams), want_undistorted=True)
            keep(f'mv_triangulate V={V} P={P}', tri.joints, tri.conf, tri.report, tri.inliers, tri.keypoints_und)
            keep(f'mv_residuals V={V} P={P}', multiview.view_residuals(tri.joints, k, dev(cams)))
        if V == 2:      # [N, J] as recorded: the sweep's brackets are neighbouring frames
            k = dev(kp)
            keep('sync_pair_sweep V=2 N=48 J=22', sync.pair_sweep(k, dev(cams), dev(pairs), dev(E_true), dev(np.array([[0.0, 0.5, -1.25, 7.0]] * Q))))

    # ---- quality ----
    for N in POINTS:
        g = rng(300 + N)
        j = (g.normal(0, 0.3, (N, 22, 3)) + (0, 0, 0.9)).astype(np.float32)
        j[:, 10:12, 2] = g.normal(0.02, 0.05, (N, 2))
        kp2 = np.concatenate([g.uniform(0, 1900, (N, 22, 2)), g.uniform(0, 1, (N, 22, 1))], -1).astype(np.float32)
        s2c = np.eye(4); s2c[:3, 3] = (0.1, -0.2, 3.0)
        gap = (np.arange(N) % 3 == 1).astype(np.uint8)
        if N >= 2:      # a NaN row in each group
            j[0, 5] = np.nan
            j[1, 9] = np.nan
        jr = (j + g.normal(0, 0.02, j.shape)).astype(np.float32)
        mk = (g.uniform(0, 1, (N, 22)) > 0.3).astype(np.float32)
        rows = torch.empty(N, 10, device=DEV, dtype=torch.float64)
        tot = torch.empty(2, 15, device=DEV, dtype=torch.float64)
        t = [dev(x) for x in (j, kp2, jr, mk, gap, s2c)]
        check(lib().rohm_track_quality(ptr(t[0]), N, 30.0, 2, 1, 0.0, ptr(t[5]), 1060.5, 1060.4, 951.3, 536.8, ptr(t[1]), 0.2, ptr(t[2]), ptr(t[3]), ptr(t[4]),
                                       ptr(rows), ptr(tot), stream_ptr(torch.device(DEV))), 'rohm_track_quality')
        keep(f'track_quality N={N}' + (' a NaN row in each group' if N >= 2 else ''), rows, tot)
        verts = g.normal(0, 0.5, (3, N, 3)).astype(np.float32)
        if N >= 2:
            verts[1, 1] = verts[1, 0]                                            # a tie: the lower index
            verts[2, N // 2, 2] = np.nan
        keep(f'floor_clearance V={N}', quality.floor_clearance(dev(verts), 'z', 0.0))

    # ---- fit shape moments ----
    tensors = synth.synthetic_smplx_tensors(0)
    from rohm_amd.body_model import SMPLXLayer, native_for  # noqa: E402
    nat = native_for(SMPLXLayer.from_tensors(tensors).to(DEV), torch.device(DEV))
    for N in POINTS:
        g = rng(500 + N)
        joints = (g.normal(0, 0.3, (N, FR.NJ, 3)) + (0, 0, 3.0)).astype(np.float32)
        conf = g.uniform(0.3, 1, (N, FR.NJ)).astype(np.float32)
        params = np.concatenate([g.standard_normal((N, FR.NROT)) * 0.3, g.standard_normal((N, 3)) + (0, 0, 3.0)], axis=1)
        use = (np.arange(N) % 5 != 2).astype(np.uint8)
        keep(f'fit_shape_moments N={N}', *shape_moments(nat, dev(joints), dev(conf), dev(params), dev(use)))

    # ---- AMASS and scene metrics ----
    for T in (3, 12, 145):
        g = rng(700 + T)
        B = 3
        jc = (g.normal(0, 0.3, (B, T, 22, 3)) + (0, 0, 0.9)).astype(np.float32)
        jr = (jc + g.normal(0, 0.03, jc.shape)).astype(np.float32)
        cc = (g.uniform(0, 1, (B, T, 4)) > 0.5).astype(np.float32)
        cr = g.uniform(0, 1, (B, T, 4)).astype(np.float32)
        out = torch.empty(B, 10, device=DEV, dtype=torch.float64)
        t = [dev(x) for x in (jc, jr, cc, cr)]
        check(lib().rohm_amass_metrics(ptr(t[0]), ptr(t[1]), ptr(t[2]), 4, ptr(t[3]), 4, 0b110110110110, 1, 2, B, T, ptr(out), stream_ptr(torch.device(DEV))),
              'rohm_amass_metrics')
        keep(f'amass_metrics T={T}', out)
        m = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1)); m[:, :3, 3] = g.normal(0, 1, (B, 3))
        gh = g.normal(0, 0.05, B).astype(np.float32)
        mk = (g.uniform(0, 1, (B, T, 22)) > 0.3).astype(np.float32)
        t = [dev(x) for x in (jr, m, gh, jc, mk)]
        for up, gt in ((2, False), (1, True)):
            out = torch.empty(B, 11, device=DEV, dtype=torch.float64)
            js = torch.empty(B, T, 22, 3, device=DEV, dtype=torch.float32)
            check(lib().rohm_scene_metrics(ptr(t[0]), ptr(t[1]), ptr(t[2]), up, ptr(t[3]) if gt else None, T if gt else 0, ptr(t[4]) if gt else None, ptr(js), B, T,
                                           ptr(out), stream_ptr(torch.device(DEV))), 'rohm_scene_metrics')
            keep(f'scene_metrics T={T} up={up}', out, js)

    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, **OUT)
    print('wrote', path, len(OUT), 'arrays', 'lib', os.environ.get('ROHM_HIP_LIB', 'shipped'))



def compare(parent, new, out_json):


    a, b = np.load(parent), np.load(new)
    assert sorted(a.files) == sorted(b.files), 'the two runs kept different arrays'
    cases, total, differ = {}, 0, 0
    for k in a.files:
        name = k.split('#')[0]
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, k
        bits = {1: np.uint8, 4: np.uint32, 8: np.uint64}[x.dtype.itemsize]
        d = int((x.view(bits) != y.view(bits)).sum())
        c = cases.setdefault(name, {'elements': 0, 'differ': 0})
        c['elements'] += int(x.size)
        c['differ'] += d
        total += int(x.size)
        differ += d
    entry = {}
    for name, c in cases.items():
        e = entry.setdefault(name.split(' ')[0], {'cases': 0, 'elements': 0, 'differ': 0})
        e['cases'] += 1
        e['elements'] += c['elements']
        e['differ'] += c['differ']
    out = {'what': 'every entry point over csrc/reduce.h, the parent commit\'s library (scripts/build_variant.py, ROHM_HIP_LIB) against this tree\'s on '
                   'identical inputs on one MI355X, all outputs compared as integers',
           'elements': total, 'differ': differ, 'entry_points': entry, 'cases': cases}
    json.dump(out, open(out_json, 'w'), indent=1)
    print(json.dumps({'elements': total, 'differ': differ, 'entry_points': entry}, indent=1))
    return 1 if differ else 0



if __name__ == '__main__':
    sys.exit(run(sys.argv[2]) if sys.argv[1] == 'run' else compare(*sys.argv[2:5]))
