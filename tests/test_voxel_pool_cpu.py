"""Voxel pooling, the parts that need no GPU: the global -> local row conversion, the C ABI's host queries, and that the fused
route declines host tensors without touching anything."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

import fv2p_native
import voxel_pool_cases as vc
from pcdet.ops.pointnet2.pointnet2_stack import voxel_pool_fused, voxel_pool_modules, voxel_query_utils

SYMBOLS = ["fv2p_voxel_pool_supported", "fv2p_voxel_pool_blocks", "fv2p_voxel_pool_saved_bytes", "fv2p_voxel_pool_ws_bytes",
           "fv2p_voxel_pool_backward_ws_bytes", "fv2p_voxel_pool_forward", "fv2p_voxel_pool_backward"]


def _reference_conversion(idx, empty, xyz_batch_cnt, batch_ids):
    """The conversion the reference executes (voxel_query_utils.py:97-102), as a loop over the queries."""
    out = idx.copy()
    starts = np.concatenate([[0], np.cumsum(xyz_batch_cnt)[:-1]])
    for i in range(idx.shape[0]):
        out[i] = 0 if empty[i] else idx[i] - starts[batch_ids[i]]
    return out


@pytest.mark.parametrize("ns,ms", [((40,), (25,)), ((50, 31), (17, 40)), ((20, 30, 25), (12, 0, 9))])
def test_local_rows(ns, ms):
    rng = np.random.default_rng(len(ns))
    idx, empty = vc.index_lists(rng, ms, ns, 8, 0.25)
    batch_ids = torch.tensor(np.repeat(np.arange(len(ns)), ms))
    cnt = torch.tensor(ns, dtype=torch.int32)
    starts = torch.cumsum(cnt, 0) - cnt
    before = idx.clone()
    got = voxel_query_utils.local_rows(idx, empty, starts, batch_ids)
    want = _reference_conversion(before.numpy(), empty.numpy(), np.array(ns), batch_ids.numpy())
    assert got.dtype == torch.int32 and np.array_equal(got.numpy(), want)
    assert torch.equal(idx, before), "local_rows must not write into the query's result"
    for b, n_b in enumerate(ns):   # every row is one of its own sample
        rows = got[batch_ids == b]
        assert rows.numel() == 0 or (int(rows.min()) >= 0 and int(rows.max()) < n_b)


def test_symbols_exported_and_declared():
    declared = fv2p_native.declared_symbols()
    handle = ctypes.CDLL(fv2p_native.LIB_PATH)
    for name in SYMBOLS:
        assert name in declared, f"{name} is not declared in include/fv2p_ops.h"
        assert hasattr(handle, name), f"{name} is not exported by libfv2p_ops.so"
    assert fv2p_native.lib().fv2p_abi_version() == 1


def test_host_queries():
    lib = fv2p_native.lib()
    ok = lib.fv2p_voxel_pool_supported
    assert ok(55296, 16, 32) == 1 and ok(1, 1, 4) == 1 and ok(1, 64, 128) == 1
    for m, s, c in [(0, 16, 32), (10, 0, 32), (10, 65, 32), (10, 16, 0), (10, 16, 6), (10, 16, 2), (10, 16, 132), (1 << 27, 16, 32), (-3, 16, 32)]:
        assert ok(m, s, c) == 0, (m, s, c)
        assert lib.fv2p_voxel_pool_ws_bytes(m, s, c) == 0 and lib.fv2p_voxel_pool_backward_ws_bytes(m, s, c, 100) == 0
    assert ok((1 << 27) - 1, 16, 32) == 1
    assert lib.fv2p_voxel_pool_backward_ws_bytes(100, 16, 32, 0) == 0
    assert lib.fv2p_voxel_pool_backward_ws_bytes(100, 16, 32, 1 << 26) == 0        # n * c reaches 2^31
    assert lib.fv2p_voxel_pool_backward_ws_bytes(1 << 25, 16, 64, 100) == 0        # m * c reaches 2^31
    assert lib.fv2p_voxel_pool_blocks(513) >= 3 and lib.fv2p_voxel_pool_blocks(1) == 1
    assert lib.fv2p_voxel_pool_blocks(0) == 0 and lib.fv2p_voxel_pool_blocks(-7) == 0
    assert lib.fv2p_voxel_pool_saved_bytes(32) >= (9 + 2 * 32) * 8
    last = (0, 0, 0)
    for m in [1, 2, 63, 64, 65, 255, 256, 257, 513, 1000, 4096, 55296, 55297, 200000, 1 << 20]:
        cur = (lib.fv2p_voxel_pool_ws_bytes(m, 16, 32), lib.fv2p_voxel_pool_backward_ws_bytes(m, 16, 32, 5000), lib.fv2p_voxel_pool_blocks(m))
        assert all(v > 0 for v in cur) and all(a >= b for a, b in zip(cur, last)), (m, cur, last)
        last = cur
    # the backward workspace holds g, the destinations and the scatter-add's own workspace for m * c single-channel entries
    m, c = 55296, 32
    assert lib.fv2p_voxel_pool_backward_ws_bytes(m, 16, c, 5000) >= 8 * m * c + lib.fv2p_scatter_add_ws_bytes(m * c, 1)


def _state(bn):
    return {k: v.clone() for k, v in bn.state_dict().items()}


def test_declines_host_tensors():
    d = vc.build(vc.CASES["c12"])
    conv, bn = vc.modules(d, 0.1, True)
    before = _state(bn)
    assert voxel_pool_fused.supported(d["f"], d["idx"], conv, bn, d["xyz"], d["new_xyz"]) is False
    assert voxel_pool_fused.voxel_pool_max(d["f"], d["xyz"], d["new_xyz"], d["idx"], d["empty"], conv, bn) is None
    after = _state(bn)
    assert all(torch.equal(before[k], after[k]) for k in before)
    # ... and odd modules, whatever the tensors are
    assert voxel_pool_fused._modules_ok(conv, bn)
    assert not voxel_pool_fused._modules_ok(nn.Conv2d(3, 12, 1, bias=True), bn)
    assert not voxel_pool_fused._modules_ok(nn.Conv2d(3, 12, 1, bias=False, stride=2), bn)
    assert not voxel_pool_fused._modules_ok(nn.Conv2d(4, 12, 1, bias=False), bn)
    assert not voxel_pool_fused._modules_ok(conv, nn.BatchNorm2d(12, affine=False))
    assert not voxel_pool_fused._modules_ok(conv, nn.BatchNorm2d(12, track_running_stats=False))
    assert not voxel_pool_fused._modules_ok(conv, nn.BatchNorm2d(16))
    hooked = copy.deepcopy(bn)
    hooked.register_forward_hook(lambda *a: None)
    assert not voxel_pool_fused._modules_ok(conv, hooked)
    replaced = copy.deepcopy(conv)
    replaced.forward = lambda x: x
    assert not voxel_pool_fused._modules_ok(replaced, bn)


class _StubGrouper(nn.Module):
    """Stands in for VoxelQueryAndGrouping (its query needs the GPU): groups by given global rows on the host."""

    def __init__(self, idx, empty, nsample):
        super().__init__()
        self.idx, self.empty, self.nsample, self.calls = idx, empty, nsample, 0

    def query(self, *a):
        raise AssertionError("the fused route was taken on host tensors")

    def forward(self, new_coords, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features, voxel2point_indices):
        self.calls += 1
        rows = self.idx.long()
        return features[rows].permute(0, 2, 1).contiguous(), xyz[rows].permute(0, 2, 1).contiguous(), self.empty


def test_module_on_host_takes_torch_route():
    assert voxel_pool_modules.NeighborVoxelSAModuleMSG.FUSED in (True, False)
    d = vc.build(((30,), (20,), 8, 16, 0.2))
    torch.manual_seed(0)
    mod = voxel_pool_modules.NeighborVoxelSAModuleMSG(query_ranges=[[1, 2, 2]], radii=[0.3], nsamples=[8], mlps=[[5, 16, 8]])
    mod.FUSED = True
    mod.groupers[0] = _StubGrouper(d["idx"], d["empty"], 8)
    feats = torch.randn(20, 5)
    coords = torch.zeros(30, 4, dtype=torch.int32)
    out = mod(d["xyz"], torch.tensor([20], dtype=torch.int32), d["new_xyz"], torch.tensor([30], dtype=torch.int32), coords, feats, None)
    assert mod.groupers[0].calls == 1 and out.shape == (30, 8)
    # what it computed is the grouped restatement
    want, _, _, _ = vc.module_restated(_rewound(mod), dict(features=feats, xyz=d["xyz"], new_xyz=d["new_xyz"], grad_out=torch.ones(30, 1)),
                                       [(d["idx"], d["empty"])], torch.float32)
    assert torch.allclose(out, want, rtol=1e-5, atol=1e-6)


def _rewound(mod):
    """A copy of `mod` with fresh BatchNorm statistics (the state before the one training-mode forward the test ran)."""
    c = copy.deepcopy(mod)
    for m in c.modules():
        if isinstance(m, nn.modules.batchnorm._BatchNorm):
            m.reset_running_stats()
    return c
