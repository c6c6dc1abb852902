"""The first convolution of the BEV backbone taken from the sparse tensor itself (tables in csrc/bev_entry.hip).

The reference densifies the last sparse tensor (HeightCompression, pcdet/models/backbones_2d/map_to_bev/height_compression.py:10-26:
``spconv_tensor.dense().view(B, C * D, H, W)``) and runs ``ZeroPad2d(1) + Conv2d(C * D -> Cout, 3)`` over the map
(base_bev_backbone.py:27-33).  A LiDAR frame leaves 3 - 10 % of the BEV cells active, so about 95 % of that layer's products have a zero
operand, forward, backward data and backward weights alike.  ``bev_entry_conv(sp, weight)`` computes the same map as a sparse
convolution with dense output rows: rows ``sp.features [N, C]`` at (b, z, y, x), 9 * D offsets k = z * 9 + ky * 3 + kx, all B * H * W
cells as destination rows, on the fused conv kernels (``fv2p_sparse_conv_rows`` forward and backward data,
``fv2p_sparse_conv_wgrad_pairs_fine`` for the weights).  The dense map, its fill and scatter, and ``dense()``'s gather in the backward pass
do not exist on this route.  The parameter stays the module's ``[Cout, C * D, 3, 3]`` tensor (channel c * D + z, as ``dense().view``
lays the map out); it is repacked to ``[9 * D][C][Cout]`` under autograd, so its gradient returns in the parameter's layout.

Above a fill of ``TAU`` (and for everything that is not the plain fp32 case) the op is the dense route it replaces.  CPU tensors take
the torch statement ``bev_entry_conv_torch`` (gather -> matmul -> index_add), which is also what the tests hold the kernels to.
"""
import torch
import torch.nn.functional as F
from torch.autograd import Function

import fv2p_native as _nat

from . import ops as _ops

# fill (SparseConvTensor.sparity) up to which the sparse route is taken.  Measured against dense() + MIOpen's conv, forward + backward at
# [3, 128 * 2, 200, 176] (profiles/bev_entry.txt): the sparse route is ahead at every measured fill, 0.17 of the dense route's time at
# 0.02 and still 0.80 at 0.8, so the crossover lies above 0.8, the densest map measured; 0.8 x that bound
TAU = 0.64
_CHANNELS = (16, 32, 64, 128)   # channel counts the conv dispatcher runs on whole fragments (csrc/sparse_conv.hip: whole_fragments); above: x 128
ROUTES = {"sparse": 0, "dense": 0, "torch": 0}   # calls per route since import (tests, records)


def repack_weight(weight, depth):
    """Conv2d weight [Cout, C * D, 3, 3] (channel c * D + z) -> [9 * D][C][Cout], offset k = z * 9 + ky * 3 + kx."""
    cout, cd = weight.shape[0], weight.shape[1]
    return weight.view(cout, cd // depth, depth, 3, 3).permute(2, 3, 4, 1, 0).reshape(9 * depth, cd // depth, cout)


def _geometry(sp):
    shape = [int(v) for v in sp.spatial_shape]
    if len(shape) != 3:
        raise ValueError("bev_entry_conv: a sparse tensor with spatial shape (D, H, W) expected, got %s" % (shape,))
    return (int(sp.batch_size), shape[0], shape[1], shape[2])


def _whole(c):
    return c in _CHANNELS or (c > 128 and c % 128 == 0)


def route(sp, weight, tau=None):
    """'sparse', 'dense' or 'torch': the route bev_entry_conv takes for this tensor and Conv2d weight."""
    f = sp.features
    if not f.is_cuda:
        return "torch"
    b, d, h, w = _geometry(sp)
    plain = (f.dtype == torch.float32 and weight.dtype == torch.float32 and weight.device == f.device and f.dim() == 2 and weight.dim() == 4
             and tuple(weight.shape[2:]) == (3, 3) and weight.shape[1] == f.shape[1] * d and not torch.is_autocast_enabled())
    if not plain or d > 3 or not (_whole(f.shape[1]) and _whole(weight.shape[0])):
        return "dense"
    if 9 * d * max(b * h * w, f.shape[0]) >= (1 << 31):
        return "dense"
    return "sparse" if sp.sparity <= (TAU if tau is None else tau) else "dense"


def _tables(indices, geom, want_pairs, plan):
    """-> (tab_out [K, B * H * W] with plan room behind it, tab_in [K, N], pairs, pair_num) from one native call."""
    b, d, h, w = geom
    ext = _nat.torch_ext()
    if ext is not None:
        return ext.bev_entry_tables(indices, b, d, h, w, bool(want_pairs), bool(plan))
    n, kvol, n_dst, dev = int(indices.shape[0]), 9 * d, b * h * w, indices.device
    tab_out = _ops.alloc_table(kvol, n_dst, dev)
    tab_in = torch.empty((kvol, n), dtype=torch.int32, device=dev)
    pairs = torch.empty((kvol, 2, n), dtype=torch.int32, device=dev) if want_pairs and n > 0 else None
    num = torch.empty((kvol,), dtype=torch.int32, device=dev) if pairs is not None else None
    with _nat.device_guard(dev):
        ws = _nat.workspace(_nat.lib().fv2p_bev_entry_tables_ws_bytes(n, d), dev)
        _nat.call("fv2p_bev_entry_tables", indices, n, b, d, h, w, tab_out, tab_in, pairs, num, ws, ws.numel(), _nat.stream())
        if plan:
            ws = _nat.workspace(_nat.lib().fv2p_conv_plan_ws_bytes(n_dst), dev)
            _nat.call("fv2p_conv_plan_build", tab_out, kvol, n_dst, ws, ws.numel(), _nat.stream())
    return tab_out, tab_in, pairs, num


def _transpose(x, batch, rows, cols):
    """[batch][rows][cols] -> [batch][cols][rows] (fv2p_transpose_batched)."""
    out = torch.empty((batch, cols, rows), dtype=x.dtype, device=x.device)
    with _nat.device_guard(x.device):
        _nat.call("fv2p_transpose_batched", x, batch, rows, cols, out, _nat.stream())
    return out


class _BevEntryConv(Function):
    """(features [N, C], w_k [9 D][C][Cout]) -> map [B, Cout, H, W]."""

    @staticmethod
    def forward(ctx, features, w_k, indices, geom):
        b, d, h, w = geom
        n, c = features.shape
        kvol, _, cout = w_k.shape
        n_dst = b * h * w
        ctx.geom, ctx.shapes = geom, (n, c, cout)
        if n == 0 or n_dst == 0:
            ctx.save_for_backward()
            return features.new_zeros((b, cout, h, w))
        features, w_k = features.contiguous(), w_k.contiguous()
        # the K-split kernel reads a tiling plan up to 65 536 destination rows (csrc/sparse_conv.hip: plan_pick_level)
        plan = c in _ops._PLAN_CHANNELS and n_dst <= 65536
        tab_out, tab_in, pairs, num = _tables(indices, geom, ctx.needs_input_grad[1], plan)
        rows = _ops._conv_rows(features, w_k, tab_out, _ops.TAB_PLANNED if plan else 0, n_dst, cout, False)
        ctx.save_for_backward(features, w_k, tab_in, pairs, num)
        return _transpose(rows, b, h * w, cout).view(b, cout, h, w)

    @staticmethod
    def backward(ctx, dy):
        b, d, h, w = ctx.geom
        n, c, cout = ctx.shapes
        kvol = 9 * d
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not ctx.saved_tensors:
            return (dy.new_zeros((n, c)) if need_x else None), (dy.new_zeros((kvol, c, cout)) if need_w else None), None, None
        features, w_k, tab_in, pairs, num = ctx.saved_tensors
        g = _transpose(dy.contiguous(), b, cout, h * w).view(b * h * w, cout)   # dY as rows, once for both gradients
        dx = dw = None
        if need_x:
            if cout in _ops._PLAN_CHANNELS and c % 64 == 0 and c <= 128:
                # the K-split tile's shapes: W_k^T materialised once and read as a plain weight (as indice_conv_backward does)
                dx = _ops._conv_rows(g, w_k.transpose(1, 2).contiguous(), tab_in, 0, n, c, False)
            else:
                dx = _ops._conv_rows(g, w_k, tab_in, 0, n, c, True)
        if need_w:
            dw = torch.empty_like(w_k)
            with _nat.device_guard(g.device):
                ws = _nat.workspace(_nat.lib().fv2p_sparse_conv_wgrad_pairs_ws_bytes(n, c, cout, kvol), g.device)
                # the `_fine` form: 16-pair chains folded in float64 - this layer's dW is held to MIOpen's blocked sums
                _nat.call("fv2p_sparse_conv_wgrad_pairs_fine", features, n, c, g, g.shape[0], cout, pairs, num, kvol, n, 0, dw, ws, ws.numel(),
                          _nat.stream())
        return dx, dw, None, None


def bev_entry_conv_torch(features, indices, geom, weight):
    """The op as torch statements: per offset gather the rows that have a cell, multiply by W_k, index_add into the cells' rows."""
    b, d, h, w = geom
    w_k = repack_weight(weight, d)
    cout = w_k.shape[2]
    out = features.new_zeros((b * h * w, cout))
    ib, iz, iy, ix = indices.long().unbind(1)
    for z in range(d):
        for ky in range(3):
            for kx in range(3):
                oy, ox = iy + 1 - ky, ix + 1 - kx
                sel = ((iz == z) & (oy >= 0) & (oy < h) & (ox >= 0) & (ox < w)).nonzero().squeeze(1)
                out = out.index_add(0, (ib[sel] * h + oy[sel]) * w + ox[sel], features[sel] @ w_k[z * 9 + ky * 3 + kx])
    return out.view(b, h, w, cout).permute(0, 3, 1, 2).contiguous()


def dense_route(sp, weight):
    """What the op replaces: HeightCompression + the zero-padded 3 x 3 convolution."""
    dense = sp.dense()
    return F.conv2d(dense.view(dense.shape[0], dense.shape[1] * dense.shape[2], dense.shape[3], dense.shape[4]), weight, None, 1, 1)


def bev_entry_conv(sp, weight, tau=None):
    """F.conv2d(sp.dense().view(B, C * D, H, W), weight, None, 1, 1) for a SparseConvTensor `sp` with spatial shape (D, H, W), rows unique
    per cell, and a Conv2d weight [Cout, C * D, 3, 3]: the sparse route up to a fill of `tau` (default TAU) on float32 CUDA tensors,
    the dense route otherwise, the torch statement on the CPU."""
    r = route(sp, weight, tau)
    ROUTES[r] += 1
    if r == "dense":
        return dense_route(sp, weight)
    geom = _geometry(sp)
    if r == "torch":
        return bev_entry_conv_torch(sp.features, sp.indices, geom, weight)
    return _BevEntryConv.apply(sp.features, repack_weight(weight, geom[1]), sp.indices.contiguous(), geom)
