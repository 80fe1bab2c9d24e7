"""Host: the predicate behind the chain's and the stack's 32-bit lane offsets (rohm_posenet_stack_addressable, csrc/encoder_chain.hip
encoder_chain_addressable; plan_encoder falls back to one launch per GEMM where it says no).  Made-up sizes, nothing is allocated or
launched: every operand -- activations of M rows and max(3 D, F, k_pack) columns, weights of max(3 D, F) rows and max(D, F, k_pack)
columns, 4 bytes an element -- must be smaller than 2^31 bytes."""
import pytest


def _fits(M, D=512, F=1024, KP=608):
    from rohm_amd._lib import lib
    return lib().rohm_posenet_stack_addressable(M, D, F, KP)


def _restated(M, D, F, KP):
    cols = max(3 * D, F, KP)
    return int(M > 0 and D > 0 and F > 0 and KP >= 0 and 4 * M * cols < 2 ** 31 and 4 * max(3 * D, F) * max(D, F, KP) < 2 ** 31)


def test_the_supported_domain_fits():
    for B in (1, 25, 32, 48, 64, 128, 1024):
        assert _fits(B * 144) == 1
    assert 4 * 128 * 144 * 1536 == 113246208          # the largest operand at B = 128: 113 MB


def test_the_bound_is_two_to_the_31_bytes_per_operand():
    edge = 2 ** 31 // (4 * 1536)                      # the most rows of [M, 3 D] under 2^31 bytes (2^31 is no multiple of a row)
    assert 4 * edge * 1536 < 2 ** 31 <= 4 * (edge + 1) * 1536
    assert _fits(edge - 1) == 1 and _fits(edge) == 1 and _fits(edge + 1) == 0
    assert _fits(2 ** 31 // (4 * 4096) - 1, F=4096) == 1 and _fits(2 ** 31 // (4 * 4096), F=4096) == 0      # ff is the widest
    assert _fits(144, KP=2 ** 20) == 0 and _fits(144, KP=2 ** 17) == 1                                    # the packed input / w_fold
    assert _fits(144, D=16384, F=16384) == 0                                                              # a weight alone


def test_nonsense_and_overflowing_sizes_are_refused():
    assert _fits(0) == 0 and _fits(-144) == 0 and _fits(144, D=0) == 0 and _fits(144, F=-1) == 0 and _fits(144, KP=-1) == 0
    assert _fits(2 ** 62) == 0 and _fits(2 ** 40, D=2 ** 30, F=2 ** 30, KP=2 ** 30) == 0


@pytest.mark.parametrize('M, D, F, KP', [(144, 512, 1024, 608), (349524, 512, 1024, 320), (349525, 512, 1024, 320), (349526, 512, 1024, 320),
                                         (10 ** 6, 128, 256, 64), (10 ** 7, 128, 256, 64), (4608, 2048, 8192, 608), (9216, 512, 1024, 70000)])
def test_the_library_agrees_with_the_restated_rule(M, D, F, KP):
    assert _fits(M, D, F, KP) == _restated(M, D, F, KP)
