"""The encoder stack at 4 parts per clip (B >= 48) with head-aligned in-projection tiles (csrc/encoder_chain.hip gemm_phase HEAD):
part tn computes head tn's q | k | v and hands them to its attention item through LDS, so qkv never goes through memory and no
meeting precedes attention.  Against the launch-per-GEMM path, at a full round of workgroups (B = 64) and a partial one (B = 50),
run after run, and through the fallback when an exchange of the stack is sabotaged."""
import pytest
import torch

from helpers import cpu_noise_sequence, seeded
from test_gpu_chain import _inputs, _pair
from test_gpu_posenet import DEV, make_diffusion, make_posenet

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('B', [64, 50])
def test_head_local_stack_matches_one_launch_per_gemm(B, monkeypatch):
    plain, net = _pair(monkeypatch, chain='stack', any_batch=True)
    x, c, t = _inputs(B)
    want = plain({'x_t': x, 'cond': c}, t)
    got = net({'x_t': x, 'cond': c}, t)
    net.check_exchange()
    diff = (got - want).abs()
    print(f'B={B} head-local stack: max|stack - launches| = {float(diff.max()):.3e}, {int((diff > 0).sum())} of {diff.numel()} differ')
    assert float(diff.max()) < 2e-5
    for _ in range(20):      # the K / Q / V handoff goes through three barriers of one workgroup: every run the same bits
        assert torch.equal(net({'x_t': x, 'cond': c}, t), got)
    net.check_exchange()


def test_head_local_stack_loop_survives_a_failed_exchange(monkeypatch):
    """The stack's first LayerNorm exchange sabotaged at B = 64 (4 parts per clip): the loop falls back to one launch per GEMM and
    repeats the chunk -- the result of a handle that never used the exchanging launches."""
    with monkeypatch.context() as m:
        m.setenv('ROHM_POSENET_LN_FUSED', '0')
        m.setenv('ROHM_POSENET_HEAD_SK', '0')
        plain, _ = make_posenet(5)
        assert plain.native(torch.device(DEV)).exchange_mode == 0
    _, net = _pair(monkeypatch, chain='stack')
    B = 64
    cond = seeded(4, B, 294, 1, 143).to(DEV)
    x_T, noises = cpu_noise_sequence(9, (B, 294, 1, 143), 6)

    def run(n):
        diff = make_diffusion(6)
        diff.fused_chunk = 3
        diff.noise_source = lambda step, like: (x_T if step == -1 else noises[step])
        return diff.p_sample_loop(n, {'cond': cond}, [B, 294, 1, 143])
    want = run(plain)
    nat = net.native(torch.device(DEV))
    nat.inject_exchange_fault(1)
    with pytest.warns(UserWarning, match='ran into its bound'):
        got = run(net)
    assert nat.exchange_mode & 51 == 0 and nat.exchange_mode & 8
    assert torch.equal(got, want)
