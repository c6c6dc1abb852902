"""CPU: the 16-bit BatchNorm1d / max-pool entry points exist in header and library, their workspace query is a host function, and the
cases of bn_half_cases.py satisfy the conditions under which the GPU test may ask for bit-for-bit equality (exact cases) or may
exclude a flipped ReLU mask (random cases)."""
import ctypes

import numpy as np
import pytest
import torch

import fv2p_native as nat
import bn_half_cases as cases

NEW_SYMBOLS = ["fv2p_batchnorm_h_ws_bytes", "fv2p_batchnorm_forward_h", "fv2p_batchnorm_apply_h", "fv2p_batchnorm_backward_h",
               "fv2p_sparse_maxpool_fwd_h", "fv2p_sparse_maxpool_bwd_h"]


def test_the_16_bit_entry_points_are_declared_and_exported():
    declared = nat.declared_symbols()
    raw = ctypes.CDLL(nat.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, name + " is not declared in include/fv2p_ops.h"
        assert hasattr(raw, name), name + " is not exported by libfv2p_ops.so"
    assert len(declared["fv2p_batchnorm_forward_h"].params) == 20
    assert len(declared["fv2p_batchnorm_apply_h"].params) == 13
    assert len(declared["fv2p_batchnorm_backward_h"].params) == 20
    assert len(declared["fv2p_sparse_maxpool_fwd_h"].params) == 10
    assert len(declared["fv2p_sparse_maxpool_bwd_h"].params) == 10
    assert nat.lib().fv2p_abi_version() == 1


def test_workspace_query_is_a_pure_host_function():
    lib = nat.lib()
    for c in (1, 16, 128, 1024):
        assert lib.fv2p_batchnorm_h_ws_bytes(1000, c) >= 2 * c * 8          # at least one fp64 partial pair per channel
        assert lib.fv2p_batchnorm_h_ws_bytes(0, c) == lib.fv2p_batchnorm_h_ws_bytes(10 ** 6, c)


def test_single_rounding_helper_rounds_once():
    # 1 + 2^-8 + 2^-30: above the bfloat16 tie 1 + 2^-8, but fp32 drops the 2^-30 and the second rounding would then go to even (1.0)
    v = np.array([1.0 + 2.0 ** -8 + 2.0 ** -30, -(1.0 + 2.0 ** -8 + 2.0 ** -30), 1.0 + 2.0 ** -8, 3.0, 0.0])
    assert cases.round64_to(v, torch.bfloat16).tolist() == [1.0 + 2.0 ** -7, -(1.0 + 2.0 ** -7), 1.0, 3.0, 0.0]
    w = np.array([1.0 + 2.0 ** -11 + 2.0 ** -30, 1.0 + 2.0 ** -11])
    assert cases.round64_to(w, torch.float16).tolist() == [1.0 + 2.0 ** -10, 1.0]


@pytest.mark.parametrize("n,c", cases.EXACT_SHAPES)
def test_exact_cases_are_exact(n, c):
    case = cases.exact_case(n, c)
    x = case["x"]
    assert set(np.unique(x).tolist()) == {-2.0, 2.0} and np.array_equal((x > 0).sum(0), np.full(c, n // 2))
    assert np.array_equal(x.mean(0), np.zeros(c)) and np.array_equal(x.var(0), np.full(c, 4.0))
    assert np.abs(case["gamma"]).max() <= 2 and np.abs(case["beta"]).max() <= 3 and np.abs(case["res"]).max() <= 3
    assert set(np.unique(case["dy"]).tolist()) <= {-1.0, 0.0, 1.0}
    for key, y in case["y"].items():
        assert np.array_equal(y, np.round(y)) and np.abs(y).max() <= cases.EXACT_MAX, key
        dx, dgamma, dbeta, dz = case["bwd"][key]
        assert np.array_equal(dx, case["gamma"] * 0.5 * dz), key
        assert np.array_equal(2 * dx, np.round(2 * dx)) and np.abs(dx).max() <= 1.0            # multiples of 1/2: exact in both formats
        for v in (dgamma, dbeta):
            assert np.array_equal(v, np.round(v)) and np.abs(v).max() <= cases.EXACT_MAX, key


@pytest.mark.parametrize("args", cases.random_case_ids(), ids=lambda a: "-".join(str(v).replace("torch.", "") for v in a))
def test_random_cases_keep_every_pre_activation_away_from_the_relu_kink(args):
    """A pre-activation within the kernel's fp32 evaluation error e of 0 could flip the ReLU mask, which changes dgamma / dbeta
    legitimately; such inputs are excluded by construction (cap 0).  2^-24 is added to e: a positive float16 result below it rounds to
    0, and the residual form reads its mask from the stored result."""
    case = cases.random_case(*args)
    n, c, dtype, pdtype, relu, has_res = args
    for name in ("x", "dy") + (("res",) if has_res else ()):
        assert np.array_equal(case[name], cases.round_to(case[name], dtype)), name
    for name in ("gamma", "beta"):
        assert np.array_equal(case[name], cases.round_to(case[name], pdtype)), name
    assert 0.5 <= case["gamma"].min() and case["gamma"].max() <= 1.5 and np.abs(case["beta"]).max() <= 0.5
    assert case["y"].dtype == np.float64 and np.isfinite(case["e"]).all() and (case["e"] > 0).all()
    if relu:
        assert int((np.abs(case["pre"]) <= case["e"] + cases.EPS24).sum()) == 0
