"""Inputs and the float64 reference shared by tests/test_bev_entry_cpu.py and tests/test_bev_entry_gpu.py (not a test module).

A case is (B, D, H, W, C, Cout, indices [N, 4] of unique (b, z, y, x) rows); the reference is F.conv2d in float64 on the CPU over the
densified input, dX the gradient at the active rows and dW by autograd, for one random upstream gradient."""
import functools

import torch
import torch.nn.functional as F


def _rows(cells):
    return torch.tensor(sorted(set(cells)), dtype=torch.int32).reshape(-1, 4)


def _clustered(gen, b, d, h, w, n, blobs=4):
    """About n unique rows of one sample in a few Gaussian blobs (what a LiDAR frame's BEV occupancy looks like)."""
    cy = torch.randint(0, h, (blobs,), generator=gen).float()
    cx = torch.randint(0, w, (blobs,), generator=gen).float()
    which = torch.randint(0, blobs, (2 * n,), generator=gen)
    y = (cy[which] + torch.randn(2 * n, generator=gen) * h / 8).round().long().clamp(0, h - 1)
    x = (cx[which] + torch.randn(2 * n, generator=gen) * w / 8).round().long().clamp(0, w - 1)
    z = torch.randint(0, d, (2 * n,), generator=gen)
    cells = sorted(set(zip([b] * (2 * n), z.tolist(), y.tolist(), x.tolist())))
    keep = torch.randperm(len(cells), generator=gen)[:n].tolist()
    return [cells[i] for i in keep]


def _mixed(gen, batch, h, w, per_sample, samples=None):
    """Both z planes at half of the chosen cells, only z = 1 at the others."""
    cells = []
    for b in (range(batch) if samples is None else samples):
        pick = torch.randperm(h * w, generator=gen)[:per_sample].tolist()
        for i, p in enumerate(pick):
            cells.append((b, 1, p // w, p % w))
            if i % 2 == 0:
                cells.append((b, 0, p // w, p % w))
    return cells


def _layout(name):
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    if name == "corners":       # border taps dropped
        return 1, 2, 9, 7, 128, 128, _rows([(0, 0, 0, 0), (0, 1, 0, 0), (0, 1, 8, 6)])
    if name == "mixed":         # 126 destination rows: no multiple of 16 or 64
        return 2, 2, 9, 7, 128, 128, _rows(_mixed(gen, 2, 9, 7, 14))
    if name == "empty_sample":  # the middle sample has no rows
        return 3, 2, 9, 7, 128, 128, _rows(_mixed(gen, 3, 9, 7, 10, samples=(0, 2)))
    if name == "n0":
        return 1, 2, 9, 7, 128, 128, torch.zeros((0, 4), dtype=torch.int32)
    if name == "full":          # the op equals the dense conv everywhere
        return 1, 2, 8, 8, 128, 128, _rows([(0, z, y, x) for z in range(2) for y in range(8) for x in range(8)])
    if name == "plan":          # 2 880 destination rows: the tiling plan behind the table is built and read
        return 2, 2, 40, 36, 128, 128, _rows(_clustered(gen, 0, 2, 40, 36, 150) + _clustered(gen, 1, 2, 40, 36, 150))
    if name == "d1":
        return 2, 1, 9, 7, 16, 32, _rows(_clustered(gen, 0, 1, 9, 7, 12) + _clustered(gen, 1, 1, 9, 7, 12))
    if name == "d3":
        return 2, 3, 9, 7, 16, 32, _rows(_clustered(gen, 0, 3, 9, 7, 20) + _clustered(gen, 1, 3, 9, 7, 20))
    if name == "odd_channels":  # 24 channels: no whole-fragment instance of the conv kernels, the dense route
        return 2, 2, 9, 7, 24, 32, _rows(_mixed(gen, 2, 9, 7, 6))
    if name == "dense_fill":    # fill 0.9: above any threshold of the sparse route
        cells = [(0, z, y, x) for z in range(2) for y in range(8) for x in range(8)]
        return 1, 2, 8, 8, 16, 16, _rows([cells[i] for i in torch.randperm(128, generator=gen)[:115].tolist()])
    raise KeyError(name)


def densify(features, indices, geom):
    """dense().view(B, C * D, H, W) as differentiable torch statements."""
    b, d, h, w = geom
    ind = indices.long()
    dense = features.new_zeros((b, d, h, w, features.shape[1])).index_put((ind[:, 0], ind[:, 1], ind[:, 2], ind[:, 3]), features)
    return dense.permute(0, 4, 1, 2, 3).reshape(b, features.shape[1] * d, h, w)


@functools.lru_cache(maxsize=None)
def case(name):
    """fp32 inputs on the CPU and the float64 results of one case: computed once, shared, never modified."""
    b, d, h, w, c, cout, ind = _layout(name)
    gen = torch.Generator().manual_seed(1000 + sum(map(ord, name)))
    feats = torch.randn((ind.shape[0], c), generator=gen)
    weight = torch.randn((cout, c * d, 3, 3), generator=gen) / (3.0 * (c * d) ** 0.5)
    grad = torch.randn((b, cout, h, w), generator=gen)
    f64, w64 = feats.double().requires_grad_(True), weight.double().requires_grad_(True)
    y = F.conv2d(densify(f64, ind, (b, d, h, w)), w64, None, 1, 1)
    dx, dw = torch.autograd.grad(y, [f64, w64], grad.double())
    return dict(geom=(b, d, h, w), c=c, cout=cout, indices=ind, features=feats, weight=weight, grad=grad,
                refs=dict(y=y.detach(), dx=dx, dw=dw))
