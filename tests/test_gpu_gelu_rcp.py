"""GPU: the erf-GELU of the GEMM epilogues (csrc/common.h gelu_erf, Abramowitz-Stegun 7.1.26 with the hardware reciprocal) against
float64 erf-GELU, element by element.

The values go through ONE EPI_BIAS_GELU GEMM whose products are exact -- identity weight, zero bias: every accumulator is x * 1 plus
zeros -- so the only arithmetic between input and output is gelu_erf itself.

Bar 6e-7 absolute: the formula evaluated in fp32 (numpy) against float64 erf-GELU on 2e6 points of [-8, 8] is off by at most 4.67e-7,
and stays there with the reciprocal pushed one ulp either way (what v_rcp_f32 may do); one fp32 ulp at 1.0 (1.2e-7) on top for the
hardware exp and the compiler's fma contraction."""
import pytest
import torch

from helpers import max_abs
from oracle import nets

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('M,N', [(1563, 64),      # narrow tiles, a part-filled last row tile
                                 (144 * 5, 128)])  # the 144-row tiles of the encoder's shapes
def test_gelu_epilogue_against_float64(M, N):
    from rohm_amd import ops
    d = torch.device('cuda', 0)
    n = M * N                                      # ~1e5 points, both ends and 0 included
    x = torch.linspace(-8.0, 8.0, n, dtype=torch.float64).float()
    x[n // 2] = 0.0
    a = x.reshape(M, N).contiguous()
    out = ops.gemm(a.to(d), torch.eye(N).to(d), torch.zeros(N).to(d), None, ops.EPI_BIAS_GELU).cpu()
    ref = nets.gelu_erf(a.double())
    err = max_abs(out, ref)
    print(f'gelu_erf through a {M} x {N} GEMM: max|HIP - float64| = {err:.3e}')
    assert torch.isfinite(out).all()
    assert err < 6e-7, err
