"""CPU: the 16-bit sparse conv entry points exist in header and library, their workspace query is a host function, and the exact
cases of half_cases.py satisfy the conditions under which the GPU test may ask for bit-for-bit equality."""
import ctypes

import numpy as np
import pytest

import fv2p_native as nat
import half_cases

NEW_SYMBOLS = ["fv2p_sparse_conv_rows_h", "fv2p_sparse_conv_wgrad_h_ws_bytes", "fv2p_sparse_conv_wgrad_h"]


def test_the_16_bit_entry_points_are_declared_and_exported():
    declared = nat.declared_symbols()
    raw = ctypes.CDLL(nat.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, name + " is not declared in include/fv2p_ops.h"
        assert hasattr(raw, name), name + " is not exported by libfv2p_ops.so"
    # the header's prototypes: (src, n_src, c_src, weight, kvol, tab, n_dst, c_dst, flip_k, transpose_w, bias, dst, dtype, stream)
    assert [k for k, _, _ in declared["fv2p_sparse_conv_rows_h"].params] == [
        "ptr", "scalar", "scalar", "ptr", "scalar", "ptr", "scalar", "scalar", "scalar", "scalar", "ptr", "ptr", "scalar", "scalar"]
    assert len(declared["fv2p_sparse_conv_wgrad_h"].params) == 14
    assert nat.lib().fv2p_abi_version() == 1


def test_weight_gradient_workspace_query_is_a_pure_host_function():
    lib = nat.lib()
    nbytes = lib.fv2p_sparse_conv_wgrad_h_ws_bytes(1000, 64, 64, 27)
    assert nbytes > 0
    assert nbytes >= 27 * 64 * 64 * 4                                            # at least one fp32 partial tile per offset
    assert lib.fv2p_sparse_conv_wgrad_h_ws_bytes(100000, 64, 64, 27) >= nbytes   # and no fewer for more rows
    assert lib.fv2p_sparse_conv_wgrad_h_ws_bytes(0, 64, 64, 27) > 0


@pytest.mark.parametrize("args", half_cases.exact_case_ids(), ids=lambda a: "-".join(str(v) for v in a[:4]))
def test_exact_cases_stay_inside_the_exact_integer_range_of_bfloat16(args):
    """The builder asserts it; stated here once more so that a case that leaves the range fails THIS test, on the oracle alone."""
    case = half_cases.exact_case(*args)
    for name in ("ref", "din", "dw"):
        v = case[name]
        assert np.array_equal(v, np.round(v)) and np.abs(v).max() <= half_cases.EXACT_MAX, (name, float(np.abs(v).max()))
    for name in ("feats", "g", "w"):
        assert set(np.unique(case[name]).tolist()) <= {-1.0, 0.0, 1.0}
    if case["bias"] is not None:
        assert np.abs(case["bias"]).max() <= 2
    assert case["ref"].shape == (case["n_dst"], case["cout"]) and case["din"].shape == case["feats"].shape and case["dw"].shape == case["w"].shape
