"""Voxel pooling on 16-bit rows, the parts that need no GPU: the three *_h symbols of the C ABI, the host query of the backward
workspace, and that the rounded cases keep the share of near-tie cells under the cap of voxel_pool_cases."""
import ctypes

import pytest
import torch

import fv2p_native
import voxel_pool_cases as vc
import voxel_pool_half_cases as hc

SYMBOLS = ["fv2p_voxel_pool_forward_h", "fv2p_voxel_pool_backward_h", "fv2p_voxel_pool_backward_h_ws_bytes"]
M_LIST = [1, 2, 63, 64, 65, 255, 256, 257, 513, 1000, 4096, 55296, 55297, 200000, 1 << 20]     # of test_voxel_pool_cpu.test_host_queries


def test_symbols_exported_and_declared():
    declared = fv2p_native.declared_symbols()
    handle = ctypes.CDLL(fv2p_native.LIB_PATH)
    for name in SYMBOLS:
        assert name in declared, f"{name} is not declared in include/fv2p_ops.h"
        assert hasattr(handle, name), f"{name} is not exported by libfv2p_ops.so"
    assert fv2p_native.lib().fv2p_abi_version() == 1


def test_backward_workspace_query():
    lib = fv2p_native.lib()
    h, f32, sc = lib.fv2p_voxel_pool_backward_h_ws_bytes, lib.fv2p_voxel_pool_backward_ws_bytes, lib.fv2p_scatter_add_ws_bytes
    # 0 wherever the fp32 query is 0
    for m, s, c, n in [(0, 16, 32, 100), (10, 0, 32, 100), (10, 65, 32, 100), (10, 16, 0, 100), (10, 16, 6, 100), (10, 16, 2, 100), (10, 16, 132, 100),
                       (1 << 27, 16, 32, 100), (-3, 16, 32, 100), (100, 16, 32, 0), (100, 16, 32, 1 << 26), (1 << 25, 16, 64, 100)]:
        assert f32(m, s, c, n) == 0 and h(m, s, c, n) == 0, (m, s, c, n)
    # elsewhere: g in 2 bytes and the int32 destination per cell and the scatter-add's own workspace fit, and the whole is 2 bytes per
    # cell below the fp32 one - at every size, the small ones where the regions' padding outweighs the cells included
    shapes = [(m, 16, 32, 5000) for m in M_LIST] + [(1, 1, 4, 1), (4, 3, 16, 7), (3, 2, 20, 9), (16, 64, 128, 33), (37, 5, 12, 23), ((1 << 27) - 1, 16, 8, 100)]
    for m, s, c, n in shapes:
        assert f32(m, s, c, n) > 0, (m, s, c, n)
        got = h(m, s, c, n)
        assert got >= 6 * m * c + sc(m * c, 1), (m, s, c, n, got)
        assert got <= f32(m, s, c, n) - 2 * m * c, (m, s, c, n, got, f32(m, s, c, n))
    last = 0
    for m in M_LIST:   # never decreasing in m
        cur = h(m, 16, 32, 5000)
        assert cur >= last, (m, cur, last)
        last = cur


@pytest.mark.parametrize("dtype", hc.DTYPES)
@pytest.mark.parametrize("training", [True, False])
def test_rounded_cases_stay_under_the_cap(dtype, training):
    """What the GPU tests lean on: with F and grad_out rounded, few cells of any case lie within MARGIN of a tie or of zero, and no
    positive output is small enough to round to zero in 16 bits (the stored-output ReLU mask is the fp32 op's)."""
    lowest = float("inf")
    for name, case in vc.CASES.items():
        d = hc.build(case, dtype)
        res, marg = vc.restated(d, 0.1, training, torch.float64, 1)
        share = float((marg < vc.MARGIN).double().mean())
        assert share <= vc.MAX_MASKED, (name, share)
        out = res[0]["out"]
        if bool((out > 0).any()):
            lowest = min(lowest, float(out[out > 0].min()))
    print(f"{dtype} training={training}: smallest positive output {lowest:.2e}")
    assert lowest > 2.0 ** -14, "a positive output in float16's subnormal range"
