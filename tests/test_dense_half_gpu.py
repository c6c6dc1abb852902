"""GPU: SparseConvTensor.dense() on float16 / bfloat16 features (fv2p_sparse_to_dense_h / fv2p_dense_to_sparse_h, csrc/sparse_aux.hip).

The elements are moved, never converted, so every check is bit for bit (view(torch.int16)):
  forward : equals scatter_nd + permute on the same 16-bit tensor, with the output buffer pre-filled with NaN by a freed allocation of
            the same size (the fill belongs to the call);
  backward: equals indexing the dense gradient at the active cells;
  dtypes  : the output and features.grad have the input's.
Channels 8 / 128 take the 16-byte path (channels_last), 3 / 12 the element path, 8 on a view that starts one element into its storage
is misaligned and takes the element path too.  n in {0, 1, 257}, batch 2, grids [3, 5, 7] and [6, 9]; the last row sits in the very last
cell of the last sample."""
import numpy as np
import pytest
import torch

import pcdet.ops.spconv as spconv
from pcdet.ops.spconv.structure import scatter_nd
from exit_half_util import DTYPES, bits, dtype_id, missing_symbols

pytestmark = pytest.mark.gpu
BATCH = 2
GRIDS = {3: [3, 5, 7], 2: [6, 9]}


@pytest.fixture(autouse=True)
def _needs_the_16_bit_entry_points():
    missing = missing_symbols()
    assert not missing, "libfv2p_ops.so lacks %s: nothing is launched" % ", ".join(missing)


def _indices(n, ndim, seed):
    grid = GRIDS[ndim]
    cells = BATCH * int(np.prod(grid))
    rng = np.random.default_rng(seed)
    if n - 1 <= cells - 1:
        flat = np.sort(rng.choice(cells - 1, size=max(n - 1, 0), replace=False)) if n > 1 else np.zeros((0,), np.int64)
    else:   # more rows than cells (257 rows on the 108 cells of the 2-D grid): every cell, then repeats; _same_rows makes the repeats equal
        flat = np.sort(np.concatenate([np.arange(cells - 1), rng.integers(0, cells - 1, size=n - cells)]))
    if n >= 1:
        flat = np.concatenate([flat, [cells - 1]])          # the very last cell of the last sample
    coords = np.stack(np.unravel_index(flat.astype(np.int64), [BATCH] + grid), axis=1) if n else np.zeros((0, ndim + 1))
    return torch.from_numpy(np.ascontiguousarray(coords, dtype=np.int32))


def _same_rows(feats, ind):
    """Rows that share a cell get the features of the first of them: whichever writer wins, the result is the same."""
    _, first, inverse = np.unique(ind.numpy(), axis=0, return_index=True, return_inverse=True)
    return feats[torch.from_numpy(first[inverse.reshape(-1)])]


def _reference(feats, ind, grid, channels_first):
    res = scatter_nd(ind.long(), feats, [BATCH] + list(grid) + [feats.shape[1]])
    if not channels_first:
        return res
    ndim = len(grid)
    perm = list(range(ndim + 1))
    perm.insert(1, ndim + 1)
    return res.permute(*perm).contiguous()


@pytest.mark.parametrize("n", [0, 1, 257])
@pytest.mark.parametrize("c,offset", [(8, 0), (128, 0), (3, 0), (12, 0), (8, 1)], ids=["c8", "c128", "c3", "c12", "c8-misaligned"])
@pytest.mark.parametrize("channels_first", [True, False], ids=["cf", "cl"])
@pytest.mark.parametrize("ndim", [3, 2])
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_forward_and_backward_are_bit_exact_copies(gpu, dtype, ndim, channels_first, c, offset, n):
    grid = GRIDS[ndim]
    ind_cpu = _indices(n, ndim, 100 * n + c)
    ind = ind_cpu.to(gpu)
    g = torch.Generator().manual_seed(7 * n + c + ndim)
    rows = _same_rows(torch.randn((n, c), generator=g).to(dtype), ind_cpu) if n else torch.zeros((0, c), dtype=dtype)
    store = torch.cat([torch.zeros(offset, dtype=dtype), rows.reshape(-1)]).to(gpu)
    feats = store[offset:].view(n, c)
    assert feats.is_contiguous() and (feats.data_ptr() % 16 == 0) == (offset == 0 or n == 0)
    feats.requires_grad_(True)
    ref = _reference(feats.detach(), ind, grid, channels_first)
    numel = ref.numel()
    junk = torch.full((numel,), float("nan"), dtype=dtype, device=gpu)
    del junk                                     # the caching allocator hands these bytes to the output below
    out = spconv.SparseConvTensor(feats, ind, grid, BATCH).dense(channels_first=channels_first)
    assert out.dtype == dtype and out.shape == ref.shape
    assert np.array_equal(bits(out), bits(ref))
    dgrad = torch.randn(ref.shape, generator=g).to(dtype).to(gpu)
    out.backward(dgrad)
    assert feats.grad.dtype == dtype and feats.grad.shape == (n, c)
    moved = dgrad if not channels_first else dgrad.permute(*([0] + list(range(2, ndim + 2)) + [1]))
    want = moved[tuple(ind[:, i].long() for i in range(ndim + 1))]
    assert np.array_equal(bits(feats.grad), bits(want.contiguous()))


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_the_native_path_is_taken(gpu, dtype):
    """One autograd node named _Dense, not the scatter_nd / permute chain of the fallback."""
    ind = _indices(5, 3, 1).to(gpu)
    feats = torch.ones((5, 8), dtype=dtype, device=gpu, requires_grad=True)
    out = spconv.SparseConvTensor(feats, ind, GRIDS[3], BATCH).dense()
    assert "_Dense" in type(out.grad_fn).__name__
