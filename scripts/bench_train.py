"""Time one PoseNet training step (train-mode forward + backward through rohm_posenet_train_forward / _backward) and the same
step through torch autograd of the fp32 oracle on the GPU.  Prints ms per step and the fraction of the 157.3 TFLOP/s fp32-MFMA
peak (3 x the forward's GEMM flops, about 5.3 GFLOP per clip at T = 143).

    python scripts/bench_train.py [--B 64] [--T 143] [--layers 8] [--steps 10] [--dropout 0.1]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=64)
    ap.add_argument('--T', type=int, default=143)
    ap.add_argument('--layers', type=int, default=8)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--dropout', type=float, default=0.1)
    ap.add_argument('--no-torch', action='store_true', help='skip the torch-autograd comparison')
    a = ap.parse_args()
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
