"""GPU: a float16 / bfloat16 backbone block and its three ways out, forward and backward, with no fp32 tensor in between.

Two clouds, about 300 active voxels on a [9, 24, 24] grid: SubMConv3d(8, 16) -> BatchNorm1d -> ReLU -> SparseConv3d(16, 32, stride 2)
-> BatchNorm1d -> ReLU after .half() / .bfloat16(); then dense() of the last level, and three_interpolate and grouping_operation of
both levels' features at 64 key points.  Every tensor produced and every .grad is 16-bit, and the outputs equal, bit for bit, those of
the same chain with each exit replaced by widen -> fp32 op -> round.  This pins the wiring; test_dense_half_gpu.py and
test_point_half_gpu.py carry the parity of each op."""
import numpy as np
import pytest
import torch

import pcdet.ops.spconv as spconv
from exit_half_util import DTYPES, bits, dtype_id, missing_symbols
from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils as pu

pytestmark = pytest.mark.gpu
BATCH, GRID, KEYS, S = 2, [9, 24, 24], 64, 16


@pytest.fixture(autouse=True)
def _needs_the_16_bit_entry_points():
    missing = missing_symbols()
    assert not missing, "libfv2p_ops.so lacks %s: nothing is launched" % ", ".join(missing)


def _chain(gpu, dtype, native):
    rng = np.random.default_rng(3)
    flat = np.sort(rng.choice(BATCH * int(np.prod(GRID)), size=300, replace=False))
    ind = torch.from_numpy(np.stack(np.unravel_index(flat, [BATCH] + GRID), 1).astype(np.int32)).to(gpu)
    torch.manual_seed(0)
    block1 = spconv.SparseSequential(spconv.SubMConv3d(8, 16, 3, padding=1, bias=False, indice_key="subm1"),
                                     torch.nn.BatchNorm1d(16, eps=1e-3, momentum=0.01), torch.nn.ReLU()).to(gpu).to(dtype)
    block2 = spconv.SparseSequential(spconv.SparseConv3d(16, 32, 3, stride=2, padding=1, bias=False, indice_key="spconv2"),
                                     torch.nn.BatchNorm1d(32, eps=1e-3, momentum=0.01), torch.nn.ReLU()).to(gpu).to(dtype)
    feats = torch.from_numpy(rng.standard_normal((300, 8))).to(dtype).to(gpu).requires_grad_(True)
    x1 = block1(spconv.SparseConvTensor(feats, ind, GRID, BATCH))
    x2 = block2(x1)
    outs = {}
    if native:
        outs["dense"] = x2.dense()
    else:
        outs["dense"] = spconv.SparseConvTensor(x2.features.float(), x2.indices, x2.spatial_shape, BATCH).dense().to(dtype)
    kcnt = torch.tensor([KEYS // 2, KEYS // 2], dtype=torch.int32, device=gpu)
    for name, x in (("l1", x1), ("l2", x2)):
        f = x.features
        cnt = torch.bincount(x.indices[:, 0].long(), minlength=BATCH).int()
        lo = int(cnt.min())
        assert lo >= 1 and f.dtype == dtype
        idx3 = torch.from_numpy(rng.integers(0, f.shape[0], size=(KEYS, 3)).astype(np.int32)).to(gpu)
        w = torch.from_numpy(rng.random((KEYS, 3)).astype(np.float32)).to(gpu)
        gidx = torch.from_numpy(rng.integers(0, lo, size=(KEYS, S)).astype(np.int32)).to(gpu)
        if native:
            outs["interp_" + name] = pu.three_interpolate(f, idx3, w)
            outs["group_" + name] = pu.grouping_operation(f, cnt, gidx, kcnt)
        else:
            outs["interp_" + name] = pu.three_interpolate(f.float(), idx3, w).to(dtype)
            outs["group_" + name] = pu.grouping_operation(f.float(), cnt, gidx, kcnt).to(dtype)
    params = list(block1.parameters()) + list(block2.parameters())
    return feats, x1, x2, outs, params


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_a_16_bit_block_and_its_exits_stay_16_bit_and_match_the_fp32_exits(gpu, dtype):
    feats, x1, x2, outs, params = _chain(gpu, dtype, True)
    _, _, _, ref, _ = _chain(gpu, dtype, False)
    assert x1.features.dtype == dtype and x2.features.dtype == dtype
    assert outs["dense"].shape[:2] == (BATCH, 32) and outs["interp_l1"].shape == (KEYS, 16) and outs["group_l2"].shape == (KEYS, 32, S)
    for name, t in outs.items():
        assert t.dtype == dtype, name
        assert bool(torch.isfinite(t.float()).all()) and bool((t != 0).any()), name
        assert np.array_equal(bits(t), bits(ref[name])), name
    torch.manual_seed(1)
    grads = []
    for name, t in outs.items():
        t.retain_grad()
        grads.append(torch.randn(t.shape, device=gpu).to(dtype))
    x1.features.retain_grad()
    x2.features.retain_grad()
    torch.autograd.backward(list(outs.values()), grads)
    for name, t in [("features", feats), ("x1", x1.features), ("x2", x2.features)] + [("param %d" % i, p) for i, p in enumerate(params)]:
        assert t.grad is not None and t.grad.dtype == dtype, name
        assert bool(torch.isfinite(t.grad.float()).all()), name
    assert bool((feats.grad != 0).any())
