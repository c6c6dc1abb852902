"""CPU: the 16-bit forms of the batch gather / grouping / interpolation exist in header and library, reject a bad dtype, a null
pointer and c = 0 with FV2P_EINVAL before anything touches a device, and size their workspaces on the host - never above the fp32
forms', which carry an fp32 staging image of the gradient where these carry a 16-bit one."""
import itertools

import pytest
import torch

import fv2p_native as nat
from batch_half_util import NEW_SYMBOLS, missing_symbols

EINVAL = -1
P = 4096          # stands for a non-null device pointer: every call below is rejected before it is looked at


def test_every_entry_point_is_declared_and_exported():
    assert missing_symbols() == []
    declared = nat.declared_symbols()
    n_params = {"fv2p_gather_points_h": 9, "fv2p_gather_points_grad_h_ws_bytes": 4, "fv2p_gather_points_grad_h": 11,
                "fv2p_group_points_batch_h": 10, "fv2p_group_points_batch_grad_h_ws_bytes": 5, "fv2p_group_points_batch_grad_h": 12,
                "fv2p_three_interpolate_batch_h": 10, "fv2p_three_interpolate_batch_grad_h_ws_bytes": 4,
                "fv2p_three_interpolate_batch_grad_h": 12}    # b, c, n, m, grad_out, idx, weight, grad_points, dtype, ws, ws_bytes, stream
    assert sorted(n_params) == sorted(NEW_SYMBOLS)
    for name, n in n_params.items():
        assert len(declared[name].params) == n, name
    assert nat.lib().fv2p_abi_version() == 1


def _calls(dtype, c, null):
    """(name, thunk) per entry point; `null` replaces every feature / gradient pointer."""
    lib = nat.lib()
    ptr = None if null else P
    return [
        ("fv2p_gather_points_h", lambda: lib.fv2p_gather_points_h(2, c, 9, 8, ptr, P, ptr, dtype, None)),
        ("fv2p_gather_points_grad_h", lambda: lib.fv2p_gather_points_grad_h(2, c, 9, 8, ptr, P, ptr, dtype, P, 1 << 30, None)),
        ("fv2p_group_points_batch_h", lambda: lib.fv2p_group_points_batch_h(2, c, 9, 4, 16, ptr, P, ptr, dtype, None)),
        ("fv2p_group_points_batch_grad_h", lambda: lib.fv2p_group_points_batch_grad_h(2, c, 9, 4, 16, ptr, P, ptr, dtype, P, 1 << 30, None)),
        ("fv2p_three_interpolate_batch_h", lambda: lib.fv2p_three_interpolate_batch_h(2, c, 9, 8, ptr, P, P, ptr, dtype, None)),
        ("fv2p_three_interpolate_batch_grad_h",
         lambda: lib.fv2p_three_interpolate_batch_grad_h(2, c, 8, 9, ptr, P, P, ptr, dtype, P, 1 << 30, None)),
    ]


@pytest.mark.parametrize("what,dtype,c,null", [("dtype", 0, 8, False), ("dtype", 3, 8, False), ("null pointer", 1, 8, True),
                                              ("bad sizes", 2, 0, False)], ids=["dtype0", "dtype3", "null", "c0"])
def test_bad_arguments_are_rejected_before_any_launch(what, dtype, c, null):
    assert missing_symbols() == []
    for name, thunk in _calls(dtype, c, null):
        assert thunk() == EINVAL, name
        assert what in nat.last_error(), (name, nat.last_error())


def test_workspace_queries_are_host_functions_monotone_non_zero_and_below_the_fp32_ones():
    assert missing_symbols() == []
    lib = nat.lib()
    pairs = [(lib.fv2p_gather_points_grad_h_ws_bytes, lib.fv2p_gather_points_grad_ws_bytes, 4),
             (lib.fv2p_group_points_batch_grad_h_ws_bytes, lib.fv2p_group_points_batch_grad_ws_bytes, 5),
             (lib.fv2p_three_interpolate_batch_grad_h_ws_bytes, lib.fv2p_three_interpolate_batch_grad_ws_bytes, 4)]
    steps = [1, 2, 7, 16, 100, 1000]
    for h, f, k in pairs:
        assert h(*([0] * k)) > 0
        base = [3, 8, 40, 15, 16][:k]
        for pos in range(k):                                  # monotone in every argument, the others held
            sizes = [h(*(base[:pos] + [v] + base[pos + 1:])) for v in steps]
            assert all(a > 0 for a in sizes) and sizes == sorted(sizes), (h.__name__, pos, sizes)
        assert h(*[1] * k) < h(*[64] * k)
        for args in itertools.product([0, 1, 5, 64], repeat=k):   # never above the fp32 form of the same sizes
            assert 0 < h(*args) <= f(*args), (h.__name__, args)
    # the RoI head's sizes: b = 384, c = 128, 512 rows - the 16-bit staging image is half the fp32 one
    g, gf = pairs[0][:2]
    assert g(384, 128, 512, 216) < gf(384, 128, 512, 216)
    assert gf(384, 128, 512, 216) - g(384, 128, 512, 216) >= 384 * 128 * 512 * 2 - 512
    g, gf = pairs[1][:2]
    assert g(384, 128, 512, 216, 32) < gf(384, 128, 512, 216, 32)
    assert gf(384, 128, 512, 216, 32) - g(384, 128, 512, 216, 32) >= 384 * 128 * 512 * 2 - 512
    g, gf = pairs[2][:2]
    assert g(384, 128, 216, 512) < gf(384, 128, 216, 512)


def test_host_tensors_of_other_dtypes_are_left_to_the_cpu_mirror_and_mixed_dtypes_raise():
    """The dtype guards judge device tensors only (oracle/backend.py answers host tensors); a gradient of another dtype than the
    forward's features is refused wherever it lives."""
    from pcdet.ops.pointnet2.pointnet2_batch import pointnet2_utils as pb
    assert pb._rows_16bit("op", torch.zeros(2, dtype=torch.float64)) is False
    assert pb._rows_16bit("op", torch.zeros(2, dtype=torch.float16)) is True
    pb._coords_f32("op", torch.zeros(2, dtype=torch.float64))
    i = torch.zeros(2, 5, dtype=torch.int32)
    for fwd, grad in ((torch.float16, torch.float32), (torch.float32, torch.bfloat16), (torch.float16, torch.bfloat16)):
        with pytest.raises(TypeError, match="one dtype"):
            pb._gather_grad({"shape": (2, 3, 4, 5), "idx": i, "dtype": fwd}, torch.zeros(2, 3, 5, dtype=grad))
        with pytest.raises(TypeError, match="one dtype"):
            pb._group_grad({"shape": (2, 3, 4, 5, 1), "idx": i, "dtype": fwd}, torch.zeros(2, 3, 5, 1, dtype=grad))
        with pytest.raises(TypeError, match="one dtype"):
            pb._interp_grad({"shape": (2, 3, 4, 5), "idx": i, "weight": None, "dtype": fwd}, torch.zeros(2, 3, 5, dtype=grad))
