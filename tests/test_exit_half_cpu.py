"""CPU: the 16-bit forms of dense(), the sparse group and the stacked grouping / interpolation exist in header and library, reject
a bad dtype, a null pointer and c = 0 with FV2P_EINVAL before anything touches a device, and size their workspaces on the host."""
import ctypes

import pytest
import torch

import fv2p_native as nat
from exit_half_util import NEW_SYMBOLS, missing_symbols

EINVAL = -1
P = 4096          # stands for a non-null device pointer: every call below is rejected before it is looked at


def test_every_entry_point_is_declared_and_exported():
    assert missing_symbols() == []
    declared = nat.declared_symbols()
    n_params = {"fv2p_sparse_to_dense_h": 11, "fv2p_dense_to_sparse_h": 11, "fv2p_sparse_group_fwd_h": 10, "fv2p_sparse_group_bwd_h": 10,
                "fv2p_group_points_stack_h": 12, "fv2p_group_points_stack_grad_h": 14, "fv2p_group_points_stack_grad_h_ws_bytes": 3,
                "fv2p_three_interpolate_stack_h": 9, "fv2p_three_interpolate_stack_grad_h": 11, "fv2p_three_interpolate_stack_grad_h_ws_bytes": 3}
    assert sorted(n_params) == sorted(NEW_SYMBOLS)
    for name, n in n_params.items():
        assert len(declared[name].params) == n, name
    assert nat.lib().fv2p_abi_version() == 1


def _calls(dtype, c, null):
    """(name, thunk) per entry point; `null` replaces every feature / gradient pointer."""
    lib = nat.lib()
    ptr = None if null else P
    sp = (ctypes.c_int * 3)(3, 5, 7)
    return [
        ("fv2p_sparse_to_dense_h", lambda: lib.fv2p_sparse_to_dense_h(ptr, P, 4, c, 3, 2, sp, 1, ptr, dtype, None)),
        ("fv2p_dense_to_sparse_h", lambda: lib.fv2p_dense_to_sparse_h(ptr, P, 4, c, 3, 2, sp, 1, ptr, dtype, None)),
        ("fv2p_sparse_group_fwd_h", lambda: lib.fv2p_sparse_group_fwd_h(ptr, 4, c, P, 27, 4, 0, ptr, dtype, None)),
        ("fv2p_sparse_group_bwd_h", lambda: lib.fv2p_sparse_group_bwd_h(ptr, 4, c, P, 27, 4, 0, ptr, dtype, None)),
        ("fv2p_group_points_stack_h", lambda: lib.fv2p_group_points_stack_h(1, 4, c, 9, 16, ptr, P, P, P, ptr, dtype, None)),
        ("fv2p_group_points_stack_grad_h", lambda: lib.fv2p_group_points_stack_grad_h(1, 4, c, 9, 16, ptr, P, P, P, ptr, dtype, P, 1 << 30, None)),
        ("fv2p_three_interpolate_stack_h", lambda: lib.fv2p_three_interpolate_stack_h(4, c, 9, ptr, P, P, ptr, dtype, None)),
        ("fv2p_three_interpolate_stack_grad_h", lambda: lib.fv2p_three_interpolate_stack_grad_h(4, c, 9, ptr, P, P, ptr, dtype, P, 1 << 30, None)),
    ]


@pytest.mark.parametrize("what,dtype,c,null", [("dtype", 0, 8, False), ("dtype", 3, 8, False), ("null pointer", 1, 8, True),
                                              ("bad sizes", 2, 0, False)], ids=["dtype0", "dtype3", "null", "c0"])
def test_bad_arguments_are_rejected_before_any_launch(what, dtype, c, null):
    assert missing_symbols() == []
    for name, thunk in _calls(dtype, c, null):
        assert thunk() == EINVAL, name
        assert what in nat.last_error(), (name, nat.last_error())


def test_workspace_queries_are_host_functions_monotone_and_non_zero():
    assert missing_symbols() == []
    lib = nat.lib()
    g, t = lib.fv2p_group_points_stack_grad_h_ws_bytes, lib.fv2p_three_interpolate_stack_grad_h_ws_bytes
    assert g(0, 0, 0) > 0 and t(0, 0, 0) > 0
    for a, b in (((10, 8, 16), (1000, 8, 16)), ((1000, 8, 16), (1000, 128, 16)), ((1000, 8, 16), (1000, 8, 32))):
        assert 0 < g(*a) <= g(*b)
    assert g(10, 8, 16) < g(100000, 128, 16)
    for a, b in (((10, 8, 5), (10000, 8, 5)), ((10000, 8, 5), (10000, 128, 5)), ((10000, 8, 5), (10000, 8, 500))):
        assert 0 < t(*a) <= t(*b)
    assert t(10, 8, 5) < t(100000, 128, 5)
    # fp32 pieces of rows that span segments only (2 per 32 entries), never an fp32 image of the gradient rows: independent of the row count
    assert t(3000, 64, 10) == t(3000, 64, 10 ** 6)


def test_group_on_an_unsupported_dtype_raises_the_worded_error():
    from pcdet.ops.spconv import ops
    f = torch.zeros((4, 8), dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="float32, float16 and bfloat16"):
        ops.indice_group(f, None, None, 4)
    with pytest.raises(NotImplementedError, match="float32, float16 and bfloat16"):
        ops.indice_group_backward(f, torch.zeros((27, 4, 8), dtype=torch.float64), None, None)
    with pytest.raises(TypeError, match="one dtype"):
        ops.indice_group_backward(f.half(), torch.zeros((27, 4, 8), dtype=torch.float32), None, None)
