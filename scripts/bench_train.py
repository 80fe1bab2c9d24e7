"""Time one PoseNet training step (train-mode forward + backward through rohm_posenet_train_forward / _backward) and the same
step through torch autograd of the fp32 oracle on the GPU.  Prints ms per step and the fraction of the 157.3 TFLOP/s fp32-MFMA
peak (3 x the forward's GEMM flops, about 5.3 GFLOP per clip at T = 143).

    python scripts/bench_train.py [--B 64] [--T 143] [--layers 8] [--steps 10] [--dropout 0.1]

--net trajnet / trajcontrol times the TrajNet step instead (rohm_trajnet_train_forward / _backward) at B = 64, T = 144 against torch
autograd of oracle.nets.trajnet_forward in fp32 on the same card, the two alternating in one process after both are warm, for at
least a second per side; trajcontrol twice: everything trainable, and only controlnet.* trainable (the fine-tune).  FLOPs count
the conv products only: 3 x the forward for an all-trainable step (forward, data gradient, weight gradient of every conv); the
frozen step counts the forward, the data gradients of the final block, diff_dec1..4 (only the up-sampled half of each concat),
diff_upsample1..4 and the ControlNet, and the weight gradients of the ControlNet alone.

    python scripts/bench_train.py --net trajcontrol [--B 64] [--T 144] [--min-seconds 1.0] [--no-torch]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import nets  # noqa: E402
from rohm_amd.model.posenet import PoseNet  # noqa: E402
from rohm_amd.utils import synth  # noqa: E402

PEAK = 157.3e12


class DS:
    pose_feat_dim, traj_feat_dim = 272, 22


def step_flops(B, T, L, D=512, F=1024, C=294, c_out=272):
    S = T + 1
    per_layer = 2 * S * D * 3 * D + 2 * 2 * S * S * D + 2 * S * D * D + 2 * 2 * S * D * F
    fwd = L * per_layer + 2 * T * 2 * C * D + 2 * T * D * c_out + 2 * 2 * D * D
    return 3.0 * B * fwd


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def trajnet_conv_flops(T, ctrl, m=512, ct=13, cc=272):
    """Per clip: {name: (forward flops, counts in the frozen-backbone backward as (data gradient share, weight gradient))}."""
    ch, zo = [m // 8, m // 4, m // 2, m], [32, m // 8, m // 4, m // 2]
    convs = {}

    def conv(name, rows, cin, cout, k, dgrad=0.0, wgrad=0.0):
        convs[name] = (2.0 * rows * cin * cout * k, dgrad, wgrad)

    def res(name, rows, cin, cout, dgrad_in=0.0, inner=0.0, wgrad=0.0):
        conv(name + '.b0', rows, cin, cout, 5, dgrad_in, wgrad)
        conv(name + '.b1', rows, cout, cout, 5, inner, wgrad)
        if cin != cout:
            conv(name + '.res', rows, cin, cout, 1, dgrad_in, wgrad)
    cin = ct
    for i in range(4):
        res(f'cond_enc{i}', T >> i, cin, ch[i])
        if i < 3:
            conv(f'cond_down{i}', T >> (i + 1), ch[i], ch[i], 3)
        cin = ch[i]
    cin = ct
    for i in range(4):
        res(f'diff_enc{i}', T >> i, cin, ch[i])
        conv(f'diff_down{i}', T >> (i + 1), 2 * ch[i], 2 * ch[i], 3)
        cin = 2 * ch[i]
    res('diff_mid1', T >> 4, 2 * m, m)
    res('diff_mid2', T >> 4, m, m)
    for i in range(4):
        conv(f'diff_up{i}', T >> i, ch[i], ch[i], 2, 1.0)                    # 4 taps, 2 per output row
        res(f'diff_dec{i}', T >> i, 2 * ch[i], zo[i], 0.5, 1.0)              # frozen: only the up-sampled half of the concat
    conv('final.b0', T, 32, 32, 5, 1.0)
    conv('final.1', T, 32, ct, 1, 1.0)
    if ctrl:
        conv('zero0', T, cc, ct, 1, 0.0, 1.0)
        cin = ct
        for i in range(4):
            res(f'ctrl_enc{i}', T >> i, cin, ch[i], 1.0, 1.0, 1.0)
            conv(f'ctrl_zero{i}', T >> i, ch[i], zo[i], 1, 1.0, 1.0)
            conv(f'ctrl_down{i}', T >> (i + 1), 2 * ch[i], 2 * ch[i], 3, 0.5, 1.0)   # the cond half of its concat is frozen
            cin = 2 * ch[i]
        res('ctrl_mid1', T >> 4, 2 * m, m, 1.0, 1.0, 1.0)
        res('ctrl_mid2', T >> 4, m, m, 1.0, 1.0, 1.0)
        conv('ctrl_zero_mid', T >> 4, m, m, 1, 1.0, 1.0)
    fwd = sum(f for f, _, _ in convs.values())
    frozen = fwd + sum(f * (d + w) for f, d, w in convs.values())
    return 3.0 * fwd, frozen


def alternate(fa, fb, min_seconds, warmup):
    """ms per call of fa and fb, alternating single calls (device-synchronised host clock) until both have run min_seconds."""
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    ta = tb = 0.0
    n = 0
    while ta < min_seconds or tb < min_seconds:
        for which, fn in ((0, fa), (1, fb)):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if which == 0:
                ta += dt
            else:
                tb += dt
        n += 1
    return ta * 1e3 / n, tb * 1e3 / n, n


def main_trajnet(a):
    from rohm_amd import _lib
    from rohm_amd.model.trajnet import TrajNet
    dev = 'cuda:0'
    ctrl = a.net == 'trajcontrol'
    T = 144 if a.T == 143 else a.T
    net = TrajNet(time_dim=32, mid_dim=512, cond_dim=13, traj_feat_dim=13, trajcontrol=ctrl, device=dev)
    sd = synth.trajnet_state_dict(0, trajcontrol=ctrl)
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).train()
    g = torch.Generator().manual_seed(0)
    x, c, cot = (torch.randn(a.B, T, 13, generator=g).to(dev) for _ in range(3))
    cc = torch.randn(a.B, T, 272, generator=g).to(dev)
    t = torch.randint(0, 100, (a.B,), generator=g).to(dev)
    batch = {'x_t': x, 'cond': c, 'control_cond': cc}
    sdg = {k: v.to(dev) for k, v in sd.items()}
    all_flops, frozen_flops = (B_ * a.B for B_ in trajnet_conv_flops(T, ctrl))
    for config in (['all'] + (['controlnet_only'] if ctrl else [])):
        for k, p in net.named_parameters():
            p.requires_grad = config == 'all' or k.startswith('controlnet.')
        for k, v in sdg.items():
            v.requires_grad_(config == 'all' or k.startswith('controlnet.'))

        def native():
            net.zero_grad(set_to_none=True)
            (net(batch, t) * cot).sum().backward()

        def eager():
            for v in sdg.values():
                v.grad = None
            with torch.device(dev):      # the oracle builds its frequency table with a default-device factory call
                out = nets.trajnet_forward(sdg, x, c, t, control_cond=cc if ctrl else None)
            (out * cot).sum().backward()
        flops = all_flops if config == 'all' else frozen_flops
        if a.no_torch:
            ms, ms_t = timed(native, a.steps, a.warmup), None
        else:
            ms, ms_t, n = alternate(native, eager, a.min_seconds, a.warmup)
        res = dict(net=a.net, trainable=config, B=a.B, T=T, step_gflop=flops / 1e9, native_ms=ms, native_tflops=flops / ms / 1e9,
                   native_peak_fraction=flops / ms / 1e9 / (PEAK / 1e12), backward_gemm_launches=_lib.lib().rohm_trajnet_train_last_gemms())
        if ms_t is not None:
            res.update(torch_autograd_ms=ms_t, torch_tflops=flops / ms_t / 1e9, alternations=n)
        print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--net', choices=['posenet', 'trajnet', 'trajcontrol'], default='posenet')
    ap.add_argument('--min-seconds', type=float, default=1.0, help='TrajNet: least time measured per side')
    ap.add_argument('--B', type=int, default=64)
    ap.add_argument('--T', type=int, default=143)
    ap.add_argument('--layers', type=int, default=8)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--dropout', type=float, default=0.1)
    ap.add_argument('--no-torch', action='store_true', help='skip the torch-autograd comparison')
    a = ap.parse_args()
    if a.net != 'posenet':
        return main_trajnet(a)
    dev = 'cuda:0'
    net = PoseNet(DS(), 294, latent_dim=512, ff_size=1024, num_layers=a.layers, num_heads=4, dropout=a.dropout,
                  traj_feat_dim=22, body_model_path=torch.nn.Identity(), device=dev)
    sd = synth.posenet_state_dict(0, num_layers=a.layers)
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).train()
    g = torch.Generator().manual_seed(0)
    x = torch.randn(a.B, 294, 1, a.T, generator=g).to(dev)
    c = torch.randn(a.B, 294, 1, a.T, generator=g).to(dev)
    t = torch.randint(0, 1000, (a.B,), generator=g).to(dev)
    cot = torch.randn(a.B, 294, 1, a.T, generator=g).to(dev)

    def native():
        net.zero_grad(set_to_none=True)
        (net({'x_t': x, 'cond': c}, t) * cot).sum().backward()

    flops = step_flops(a.B, a.T, a.layers)
    ms = timed(native, a.steps, a.warmup)
    res = dict(B=a.B, T=a.T, layers=a.layers, dropout=a.dropout, step_gflop=flops / 1e9, native_ms=ms,
               native_tflops=flops / ms / 1e9, native_peak_fraction=flops / ms / 1e9 / (PEAK / 1e12))
    if not a.no_torch:
        sdg = {k: v.to(dev).requires_grad_(k != 'sequence_pos_encoder.pe') for k, v in sd.items()}

        def eager():
            for v in sdg.values():
                v.grad = None
            (nets.posenet_forward(sdg, x, c, t) * cot).sum().backward()
        ms_t = timed(eager, a.steps, a.warmup)
        res.update(torch_autograd_ms=ms_t, torch_tflops=flops / ms_t / 1e9)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
