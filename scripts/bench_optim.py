"""Time one optimiser step over the real parameter sets (PoseNet with 8 layers, TrajControl; rohm_amd.utils.synth) three ways:

  native       rohm_amd.optim.AdamW: rohm_adamw_step, one fused pass, the tensor table as kernel arguments;
  torch        torch.optim.AdamW as the loops construct it (its default form: several foreach passes);
  torch_fused  torch.optim.AdamW(fused=True), when the installed torch offers it on this device;

and the same with gradient clipping at max_norm 1.0: native with max_grad_norm (rohm_grad_norm, then the step reads the
coefficient from device memory) against torch.nn.utils.clip_grad_norm_ followed by the step.  The gradients are fixed; the forms
take turns in one process, in windows of about 0.1 s that end in a device synchronise, until each has at least --min-seconds
(scripts/bench_train_loop.py::alternate).  Reported per form: ms per step (mean, and the least and greatest window), launches
per step, the bytes an AdamW step must move (28 per element: read p, g, m, v, write p, m, v) and the rate they give as a
fraction of the 6.29 TB/s a float4 copy reaches on the MI355X.  The step time includes the host side of the call.

    python scripts/bench_optim.py [--min-seconds 1.0] [--out profiles/optim_timing.json]
    python scripts/bench_optim.py --parity [--parity-out profiles/adamw_parity.json] [--no-timing]

--parity runs the parity case of tests/optim_ref.py and records, per quantity, the native error and torch-fp32's own error against
the float64 run and their ratio (the tests' bar is 4), plus the native result's deviation from torch's fp32 AdamW on this GPU
(informative, no bar).  Needs the GPU: there is no CPU fallback and no number without a run.
"""
import argparse
import importlib.util
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rohm_amd import _lib, optim  # noqa: E402
from rohm_amd.utils import synth  # noqa: E402

COPY_RATE = 6.29e12      # bytes/s, float4 copy on the MI355X
BYTES_PER_ELEMENT = 28
MAX_NORM = 1.0


def alternate(sides, min_seconds, window=0.1):
    """{name: fn} -> {name: dict(ms, ms_min, ms_max, calls, windows)}: the sides take turns in windows of about `window` seconds
    (calls per window sized per side from one timed call), every window closed by a synchronise, until each has min_seconds."""
    chunk = {}
    for name, fn in sides.items():
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        chunk[name] = max(1, min(1000, int(window / max(time.perf_counter() - t0, 1e-6))))
    total, calls, per_window = {k: 0.0 for k in sides}, {k: 0 for k in sides}, {k: [] for k in sides}
    while min(total.values()) < min_seconds:
        for name, fn in sides.items():
            t0 = time.perf_counter()
            for _ in range(chunk[name]):
                fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            total[name] += dt
            calls[name] += chunk[name]
            per_window[name].append(dt * 1e3 / chunk[name])
    return {k: dict(ms=total[k] * 1e3 / calls[k], ms_min=min(per_window[k]), ms_max=max(per_window[k]), calls=calls[k],
                    windows=len(per_window[k])) for k in sides}


def parameter_sets():
    pose = synth.posenet_state_dict(0, num_layers=8)
    traj = synth.trajnet_state_dict(0, trajcontrol=True)
    return {'posenet_8_layers': [v for k, v in pose.items() if v.is_floating_point() and not k.endswith('.pe')],
            'trajcontrol': [v for v in traj.values() if v.is_floating_point()]}


def make_params(tensors, dev, seed):
    g = torch.Generator().manual_seed(seed)
    ps = [t.to(dev).clone().requires_grad_() for t in tensors]
    for p in ps:
        p.grad = (torch.randn(p.shape, generator=g) * 1e-3).to(dev)
    return ps


def native_launches(opt):
    """Launches of one native step, counted by the library's own launch profiler."""
    _lib.profile_start(1)
    opt.step()
    rows = _lib.profile_stop()
    return {k: v['launches'] for k, v in rows.items()}, sum(v['launches'] for v in rows.values())


def torch_launches(fn):
    """Device kernels of one call, counted by torch's profiler; None when it gives nothing on this build."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
        return n or None
    except Exception as exc:      # noqa: BLE001  (a missing tracer must not lose the timings)
        print(f'torch profiler unavailable: {exc}', flush=True)
        return None


def timing(a, dev):
    result = {'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'min_seconds': a.min_seconds,
              'bytes_per_element': BYTES_PER_ELEMENT, 'copy_rate_TBps': COPY_RATE / 1e12, 'max_norm': MAX_NORM,
              'limits': dict(zip(('tensors_per_launch', 'elems_per_block'), optim.limits())), 'sets': {}}
    pending = []
    for name, tensors in parameter_sets().items():
        elements = sum(t.numel() for t in tensors)
        nbytes = BYTES_PER_ELEMENT * elements
        entry = {'tensors': len(tensors), 'elements': elements, 'step_bytes': nbytes,
                 'least_ms_at_copy_rate': nbytes / COPY_RATE * 1e3}
        for clip in (False, True):
            opts, sides = {}, {}
            ps = make_params(tensors, dev, 1)
            opts['native'] = optim.AdamW(ps, lr=1e-4, weight_decay=0.01, max_grad_norm=MAX_NORM if clip else None)
            forms = {'torch': {}}
            try:
                torch.optim.AdamW(make_params(tensors[:1], dev, 1), fused=True).step()
                forms['torch_fused'] = {'fused': True}
            except Exception as exc:      # noqa: BLE001
                entry['torch_fused_unavailable'] = str(exc)
            sides['native'] = opts['native'].step
            for form, kw in forms.items():
                pt = make_params(tensors, dev, 1)
                opts[form] = torch.optim.AdamW(pt, lr=1e-4, weight_decay=0.01, **kw)
                if clip:
                    sides[form] = lambda o=opts[form], pt=pt: (torch.nn.utils.clip_grad_norm_(pt, MAX_NORM), o.step())
                else:
                    sides[form] = opts[form].step
            t = alternate(sides, a.min_seconds)
            for form, row in t.items():
                row['fraction_of_copy_rate'] = nbytes / (row['ms'] * 1e-3) / COPY_RATE
                row['GBps'] = nbytes / (row['ms'] * 1e-3) / 1e9
            by_kernel, n = native_launches(opts['native'])
            t['native']['launches'], t['native']['launches_by_kernel'] = n, by_kernel
            entry['clipped' if clip else 'plain'] = t
            pending += [(t[form], sides[form]) for form in forms]
            print(name, 'clipped' if clip else 'plain', {k: round(v['ms'], 4) for k, v in t.items()}, flush=True)
        result['sets'][name] = entry

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(result, f, indent=1)
    # torch's launch counts come from torch.profiler, which slows the host: it runs after the timed windows, one step per form,
    # and the timings are on disk first so that a build without a working tracer still leaves them
    write()
    if not a.no_torch_launches:
        for row, fn in pending:
            row['launches'] = torch_launches(fn)
        write()
    print(json.dumps(result))


def parity(a, dev):
    spec = importlib.util.spec_from_file_location('optim_ref', os.path.join(ROOT, 'tests', 'optim_ref.py'))
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)
    out = {'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'steps': R.K, 'margin': R.MARGIN,
           'shapes': [list(s) for s in R.SHAPES], 'groups': R.GROUPS, 'cases': {}}
    params, grads = R.make_inputs()
    for case, max_norm in (('plain', None), ('clipped_max_norm_0.5', 0.5)):
        r64, r32 = R.references(params, grads, max_norm=max_norm)
        ps, opt = R.run(lambda groups: optim.AdamW(groups, max_grad_norm=max_norm), params, grads, torch.float32, dev)
        res = R.results(ps, opt)
        pt, opt_t = R.run(R.torch_adamw(), params, grads, torch.float32, dev, max_norm, clip_with_torch=max_norm is not None)
        gpu32 = R.results(pt, opt_t)
        own, base = R.errors(res, r64), R.errors(r32, r64)
        out['cases'][case] = {
            'native_error_vs_float64': own, 'torch_fp32_cpu_error_vs_float64': base,
            'ratio': {q: own[q] / base[q] for q in R.QUANTITIES},
            'torch_fp32_gpu_error_vs_float64': R.errors(gpu32, r64),
            'native_deviation_from_torch_fp32_gpu': R.errors(res, gpu32),
        }
    os.makedirs(os.path.dirname(os.path.abspath(a.parity_out)), exist_ok=True)
    with open(a.parity_out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--min-seconds', type=float, default=1.0)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'optim_timing.json'))
    ap.add_argument('--parity', action='store_true')
    ap.add_argument('--parity-out', default=os.path.join(ROOT, 'profiles', 'adamw_parity.json'))
    ap.add_argument('--no-timing', action='store_true')
    ap.add_argument('--no-torch-launches', action='store_true', help='do not run torch\'s profiler for its launch counts')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_optim.py measures on the GPU; none is visible')
    dev = 'cuda:0'
    if a.parity:
        parity(a, dev)
    if not a.no_timing:
        timing(a, dev)


if __name__ == '__main__':
    main()
