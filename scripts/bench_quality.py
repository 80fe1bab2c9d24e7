"""How long scoring a stitched track takes: `track_quality` (two launches of csrc/quality.hip plus the read-back of the totals)
from host arrays (the uploads included) and from device tensors, `floor_clearance` per chunk of 256 meshes as
`export._vertex_chunks` delivers them, and the numpy restatement (tests/quality_ref.py) on the host of the same box, for a
synthetic ten-minute track: 18 000 frames at 30 fps with keypoints, an input track, a visibility mask and gaps.

Device-side times: a host clock around calls that end in a device synchronise (`track_quality` copies the totals back, which
waits for the kernels), median over `--windows` windows of `--inner` calls after a warm-up of the same shapes; the kernels
alone with HIP events around `--inner` back-to-back calls of the C entry point on tensors that are on the device already.
Host time: wall clock of one pass.  Recorded, not judged: nobody has timed another implementation of this path.

    python scripts/bench_quality.py [--out profiles/quality_bench.json] [--minutes 10] [--verts 10475]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import quality_ref as QR  # noqa: E402
from rohm_amd import _lib  # noqa: E402
from rohm_amd.quality import floor_clearance, track_quality  # noqa: E402

DEV = 'cuda:0'
SCENE2CAM = np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 0.0, -1.0, 1.0], [0.0, 1.0, 0.0, 3.5], [0.0, 0.0, 0.0, 1.0]])
CAM = (1060.0, 1060.0, 960.0, 540.0)


def synthetic_track(n, seed=0):
    """A body about 1.7 m tall wandering over the floor (z up): smooth joint motion, feet near the floor, keypoints a few
    pixels off its projection with 3 % of the frames in detector gaps, an input track 3 cm off."""
    g = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n) / 30.0
    f, ph = g.uniform(0.05, 0.6, size=(22, 3)), g.uniform(0, 2 * np.pi, size=(22, 3))
    j = g.uniform(-0.3, 0.3, size=(22, 3)) + 0.1 * np.sin(2 * np.pi * f * t[:, None, None] + ph)
    j[..., 2] += np.linspace(0.1, 1.6, 22)
    j[:, list(QR.FOOT), 2] = 0.06 + 0.08 * np.sin(2 * np.pi * 0.9 * t[:, None] + np.arange(4))
    j[..., :2] += np.stack([np.sin(0.05 * t), np.cos(0.03 * t)], axis=-1)[:, None]
    j = j.astype(np.float32)
    uv = QR.project(j, SCENE2CAM, *CAM)[0]
    kp = np.concatenate([uv + g.normal(0, 3.0, size=uv.shape), g.uniform(0.05, 1.0, size=(n, 22, 1))], axis=-1).astype(np.float32)
    gap = np.zeros(n, np.uint8)
    for s in g.integers(1, n - 13, size=n // 200):
        gap[s:s + int(g.integers(1, 13))] = 1
    kp[gap == 1] = 0.0
    mask = (g.uniform(size=(n, 22)) > 0.3).astype(np.float32) * (1 - gap)[:, None].astype(np.float32)
    return dict(joints=j, keypoints=kp, joints_ref=(j + g.normal(0, 0.03, size=j.shape)).astype(np.float32), mask_ref=mask, gap=gap)


def timed(fn, inner, windows):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        t = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) / inner * 1e3)
    return out


def events(fn, inner, windows):
    for _ in range(2):
        fn()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / inner)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'quality_bench.json'))
    ap.add_argument('--minutes', type=float, default=10.0)
    ap.add_argument('--verts', type=int, default=10475, help='vertices per mesh (SMPL-X: 10475)')
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--skip_host', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_quality.py measures on the GPU; none found')
    n = int(round(a.minutes * 60 * 30.0))
    d = synthetic_track(n)
    res = {'frames': n, 'fps': 30.0, 'gap_frames': int(d['gap'].sum()), 'verts': a.verts, 'chunk': 256, 'inner': a.inner, 'windows': a.windows}
    cam = dict(scene2cam=SCENE2CAM, focal=CAM[:2], center=CAM[2:])
    up = lambda x: torch.from_numpy(x).to(DEV)                                        # noqa: E731

    # as a caller with host arrays sees it: five uploads, two launches, the totals back
    host_call = lambda: track_quality(up(d['joints']), 30.0, 'z', 0.0, keypoints=up(d['keypoints']), joints_ref=up(d['joints_ref']),  # noqa: E731
                                      mask_ref=up(d['mask_ref']), gap=up(d['gap']), **cam)
    w = timed(host_call, a.inner, a.windows)
    res.update(track_quality_host_arrays_ms_median=round(statistics.median(w), 4), track_quality_host_arrays_ms_min=round(min(w), 4),
               track_quality_host_arrays_ms_max=round(max(w), 4))
    # ... and with the arrays on the device already (`score_recording`: they come from the export)
    dd = {k: up(v) for k, v in d.items()}
    m = up(SCENE2CAM)
    dev_call = lambda: track_quality(dd['joints'], 30.0, 'z', 0.0, keypoints=dd['keypoints'], joints_ref=dd['joints_ref'],  # noqa: E731
                                     mask_ref=dd['mask_ref'], gap=dd['gap'], scene2cam=m, focal=CAM[:2], center=CAM[2:])
    w = timed(dev_call, a.inner, a.windows)
    res.update(track_quality_device_arrays_ms_median=round(statistics.median(w), 4), track_quality_device_arrays_ms_min=round(min(w), 4),
               track_quality_device_arrays_ms_max=round(max(w), 4))
    # the two kernels alone
    lib, stream = _lib.lib(), _lib.stream_ptr(torch.device(DEV))
    rows, tot = torch.empty(n, 10, device=DEV, dtype=torch.float64), torch.empty(2, 15, device=DEV, dtype=torch.float64)
    m16 = m.reshape(16).contiguous()
    raw = lambda: lib.rohm_track_quality(dd['joints'].data_ptr(), n, 30.0, 2, 1, 0.0, m16.data_ptr(), *CAM, dd['keypoints'].data_ptr(), 0.2,  # noqa: E731
                                         dd['joints_ref'].data_ptr(), dd['mask_ref'].data_ptr(), dd['gap'].data_ptr(), rows.data_ptr(),
                                         tot.data_ptr(), stream)
    assert raw() == 0
    w = events(raw, a.inner, a.windows)
    bytes_moved = n * (4.0 * 66 * 5 + 4.0 * 22 + 1 + 2 * 80.0)
    res.update(track_quality_kernels_ms_median=round(statistics.median(w), 5), track_quality_kernels_bytes=int(bytes_moved),
               track_quality_kernels_gbps=round(bytes_moved / (statistics.median(w) * 1e-3) / 1e9, 1))

    # the mesh: one chunk of 256 frames, as export._vertex_chunks yields them
    g = torch.Generator(device='cpu').manual_seed(1)
    verts = (torch.rand(256, a.verts, 3, generator=g) * 1.8 - 0.1).to(DEV)
    w = timed(lambda: floor_clearance(verts, 'z', 0.0), a.inner, a.windows)
    res.update(floor_clearance_chunk_ms_median=round(statistics.median(w), 4), floor_clearance_chunk_ms_min=round(min(w), 4),
               floor_clearance_chunk_ms_max=round(max(w), 4))
    w = events(lambda: floor_clearance(verts, 'z', 0.0), a.inner, a.windows)
    res.update(floor_clearance_chunk_events_ms_median=round(statistics.median(w), 5),
               floor_clearance_chunk_gbps=round(256 * a.verts * 12.0 / (statistics.median(w) * 1e-3) / 1e9, 1),
               floor_clearance_chunks_per_track=-(-n // 256))

    if not a.skip_host:
        t = time.perf_counter()
        rows_ref, tot_ref = QR.track_quality(d['joints'], 30.0, 2, True, 0.0, SCENE2CAM, *CAM, keypoints=d['keypoints'], joints_ref=d['joints_ref'],
                                             mask_ref=d['mask_ref'], gap=d['gap'])
        res['host_restatement_track_quality_s'] = round(time.perf_counter() - t, 4)
        vh = verts.cpu().numpy()
        t = time.perf_counter()
        clear_ref = QR.floor_clearance(vh, 2, 0.0)
        res['host_restatement_floor_clearance_chunk_s'] = round(time.perf_counter() - t, 4)
        res['host_threads'] = torch.get_num_threads()
        q = dev_call()
        got = q.rows.cpu().numpy()
        res['rows_nan_pattern_equal'] = bool(np.array_equal(np.isnan(got), np.isnan(rows_ref)))
        res['rows_max_rel_vs_restatement'] = float(max(np.nanmax(np.abs(got[:, c] - rows_ref[:, c])) / np.nanmax(np.abs(rows_ref[:, c]))
                                                       for c in (0, 1, 4, 5, 6, 7)))
        res['counts_equal'] = bool(np.array_equal(q.totals[:, [0, 2, 4, 5, 7, 8, 10, 12, 14]], tot_ref[:, [0, 2, 4, 5, 7, 8, 10, 12, 14]]))
        res['floor_clearance_equal'] = bool(np.array_equal(floor_clearance(verts, 'z', 0.0).cpu().numpy(), clear_ref))
    print(json.dumps(res))
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
