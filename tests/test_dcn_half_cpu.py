"""Host side of the 16-bit deformable-convolution forward: the exactness conditions of tests/dcn_half_cases.py, which geometries
fv2p_dcn_forward_h takes, the dtype checks that come before any HIP call, and the new symbols."""
import pytest
import torch

import dcn_half_cases as cases
import fv2p_native as nat

SYMBOLS = ["fv2p_dcn_forward_h", "fv2p_dcn_forward_h_supported", "fv2p_transpose_batched_widen", "fv2p_transpose_batched_round"]
EINVAL = -1
GEOM = (1, 4, 4, 32, 16, 4, 4, 3, 3, 1, 1, 1, 1, 1, 1, 1)


def test_symbols_are_declared_and_exported():
    declared = nat.declared_symbols()
    lib = nat.lib()
    for name in SYMBOLS:
        assert name in declared, name
        getattr(lib, name)
    assert len(declared["fv2p_dcn_forward_h"].params) == 25


@pytest.mark.parametrize("family,g", cases.EXACT, ids=lambda v: v if isinstance(v, str) else cases.geom_id(v))
def test_exact_cases_are_exact_in_both_formats(family, g):
    """exact_case asserts the range itself; here: every operand and the result survive a round trip through both formats."""
    case = cases.exact_case(family, g)
    assert (8.0 if family == "half" else 1.0) * case["top"] <= 256.0
    for dtype in (torch.float16, torch.bfloat16):
        for name in ("x", "w", "bias", "offset", "mask", "ref"):
            assert torch.equal(case[name].to(dtype).float(), case[name]), (name, dtype)
    assert case["top"] >= 8.0   # the sums are not trivially small


def test_the_case_table_is_complete():
    assert len(cases.EXACT) == 11
    assert ("integer", cases.GEOMETRIES[5]) in cases.EXACT and ("half", cases.GEOMETRIES[5]) not in cases.EXACT
    assert cases.GEOMETRIES[4][0] // cases.GEOMETRIES[4][2] == 16


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=str)
def test_random_case_operands_are_representable_and_the_bound_is_positive(dtype):
    g = cases.GEOMETRIES[4]
    case = cases.random_case(g, dtype)
    for name in ("x", "w", "bias", "offset", "mask"):
        assert torch.equal(case[name].to(dtype).float(), case[name]), name
    assert float(case["offset"].abs().max()) < 4.0
    assert bool((case["S"] >= case["ref"].abs() - 1e-12).all())
    assert float(cases.bound(case, g, dtype).min()) > 0.0


@pytest.mark.parametrize("cin,cout,dg,want", [
    (32, 48, 1, 1), (64, 64, 2, 1), (128, 200, 4, 1), (48, 16, 3, 1), (16, 1, 1, 1), (256, 256, 4, 1), (64, 300, 1, 1), (256, 512, 16, 1),
    (32, 32, 4, 0), (8, 16, 1, 0), (40, 16, 1, 0), (48, 16, 2, 0), (64, 16, 3, 0), (32, 0, 1, 0), (0, 16, 1, 0), (32, 16, 0, 0), (24, 16, 1, 0)])
def test_supported_geometries(cin, cout, dg, want):
    assert nat.lib().fv2p_dcn_forward_h_supported(cin, cout, dg) == want


def test_bad_dtypes_are_refused_first_without_a_gpu():
    lib = nat.lib()
    for dt, om in [(0, 0), (3, 0), (-1, 0), (1, 2), (2, 1), (1, 3), (2, -1)]:
        assert lib.fv2p_dcn_forward_h(None, None, None, None, None, *GEOM, None, dt, om, None) == EINVAL
        assert "dcn_forward_h" in nat.last_error() and "dtype" in nat.last_error()
    for dt in (0, 3):
        assert lib.fv2p_transpose_batched_widen(None, dt, 1, 4, 4, None, None) == EINVAL
        assert "transpose_batched_widen" in nat.last_error() and "dtype" in nat.last_error()
        assert lib.fv2p_transpose_batched_round(None, 1, 4, 4, None, dt, None) == EINVAL
        assert "transpose_batched_round" in nat.last_error() and "dtype" in nat.last_error()
    # a good dtype reaches the next checks, still without a HIP call
    assert lib.fv2p_dcn_forward_h(None, None, None, None, None, *GEOM, None, 1, 0, None) == EINVAL
    assert "null" in nat.last_error()
    assert lib.fv2p_dcn_forward_h(None, None, None, None, None, *(GEOM[:3] + (24,) + GEOM[4:]), None, 2, 2, None) < 0
    assert "multiple of 16" in nat.last_error()
    assert lib.fv2p_dcn_forward_h(None, None, None, None, None, *((0,) + GEOM[1:]), None, 2, 2, None) == 0   # an empty batch: nothing to do
    assert lib.fv2p_transpose_batched_widen(None, 1, 1, 4, 4, None, None) == EINVAL
    assert lib.fv2p_transpose_batched_round(None, 0, 4, 4, None, 2, None) == 0


def test_a_cpu_tensor_never_takes_the_native_route():
    from pcdet.ops.DeformableConvolutionV2PyTorch import DCN
    assert DCN.NATIVE_16BIT is True
    x, w = torch.zeros(1, 32, 4, 4, dtype=torch.float16), torch.zeros(16, 32, 3, 3, dtype=torch.float16)
    assert not DCN._native_16bit(x, w, 1, 1)
    assert not DCN._native_16bit(x.float(), w.float(), 1, 1)
