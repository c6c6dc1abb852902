"""GPU parity of the fused sparse convolution (A5/A6/A7) through the pcdet.ops.spconv API.

Oracles: (1) oracle.indice_conv / indice_conv_backward — the reference's gather→mm→scatter loop restated with
torch CPU ops on the oracle rulebook; (2) torch.nn.functional.conv3d on the densified tensor (the upstream
spconv test idea that spconv/test_utils.py:144-193 was written for) — independent of any rulebook code.
Tolerance (north_star): 1e-4 relative for float features, stated per assert below."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import oracle
import pcdet.ops.spconv as spconv
from pcdet.ops.spconv import ops
from sparse_util import random_active

pytestmark = pytest.mark.gpu
RTOL = 1e-4


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-12)


def make_input(seed, batch, shape, n, cin, gpu):
    ind = random_active(seed, batch, shape, n)
    rng = np.random.default_rng(seed + 1)
    feats = rng.standard_normal((ind.shape[0], cin)).astype(np.float32)
    x = spconv.SparseConvTensor(torch.from_numpy(feats).to(gpu), torch.from_numpy(ind).to(gpu), shape, batch)
    return ind, feats, x


CHANNELS = [(4, 16), (5, 16), (16, 16), (16, 32), (32, 32), (32, 64), (64, 64), (64, 128), (128, 128), (24, 40), (3, 7), (160, 144)]


@pytest.mark.parametrize("cin,cout", CHANNELS)
def test_subm_conv_forward_backward_vs_oracle(gpu, front_end, cin, cout):
    batch, shape = 2, [9, 20, 18]
    ind, feats, x = make_input(cin * 100 + cout, batch, shape, 900, cin, gpu)
    conv = spconv.SubMConv3d(cin, cout, 3, padding=1, bias=False, indice_key="k").to(gpu)
    x.features.requires_grad_(True)
    y = conv(x)
    w = conv.weight.detach().cpu().numpy()
    _, pairs, num = oracle.indice_pairs(ind, batch, shape, [3, 3, 3], [1, 1, 1], [1, 1, 1], [1, 1, 1], subm=True)
    ref = oracle.indice_conv(feats, w, pairs, num, ind.shape[0], subm=True).numpy()
    assert y.features.shape == ref.shape
    assert rel_err(y.features.detach().cpu().numpy(), ref) < RTOL
    g = np.random.default_rng(7).standard_normal(ref.shape).astype(np.float32)
    y.features.backward(torch.from_numpy(g).to(gpu))
    din, dw = oracle.indice_conv_backward(feats, w, g, pairs, num, subm=True)
    assert rel_err(x.features.grad.cpu().numpy(), din.numpy()) < RTOL
    assert rel_err(conv.weight.grad.cpu().numpy(), dw.numpy()) < RTOL

@pytest.mark.parametrize("impl", [1, 2, 3, 4])
def test_conv_kernel_variants_agree_with_oracle(gpu, impl):
    """Every kernel variant behind fv2p_sparse_conv_rows (plain dense tile / compacted / register-staged pipeline;
    the default heuristic = LDS-DMA tile is what all other tests run) gives the oracle's features and input gradient,
    with a bias, with n_dst not a multiple of the 64-row tile and with a strided (non-symmetric) rulebook."""
    import fv2p_native
    try:
        fv2p_native.call("fv2p_sparse_conv_set_impl", impl)
        for cin, cout in [(16, 16), (32, 64), (64, 64), (64, 128), (128, 64), (24, 40)]:
            batch, shape = 2, [9, 20, 18]
            ind, feats, x = make_input(cin * 7 + cout, batch, shape, 1100, cin, gpu)
            conv = spconv.SparseConv3d(cin, cout, 3, stride=2, padding=1, bias=True).to(gpu)
            x.features.requires_grad_(True)
            y = conv(x)
            w, b = conv.weight.detach().cpu().numpy(), conv.bias.detach().cpu().numpy()
            outids, pairs, num = oracle.indice_pairs(ind, batch, shape, [3, 3, 3], [2, 2, 2], [1, 1, 1], [1, 1, 1])
            ref = oracle.indice_conv(feats, w, pairs, num, outids.shape[0]).numpy() + b
            assert rel_err(y.features.detach().cpu().numpy(), ref) < RTOL, (impl, cin, cout)
            g = np.random.default_rng(3).standard_normal(ref.shape).astype(np.float32)
            y.features.backward(torch.from_numpy(g).to(gpu))
            din, _ = oracle.indice_conv_backward(feats, w, g, pairs, num)
            assert rel_err(x.features.grad.cpu().numpy(), din.numpy()) < RTOL, (impl, cin, cout)
    finally:
        fv2p_native.call("fv2p_sparse_conv_set_impl", 0)


THIN_ROWS = [15, 16, 17, 4097, 65536, 65537]


@pytest.mark.parametrize("n_rows", THIN_ROWS)
@pytest.mark.parametrize("cin,cout", [(16, 16), (32, 32), (32, 16), (16, 32), (4, 16), (5, 16), (4, 32)])
def test_thin_layer_kernels_on_and_off_vs_oracle(gpu, cin, cout, n_rows):
    """conv_rows_thin (16 -> 16: backward data, and the forward with a source BatchNorm), conv_rows_res (32 source channels, <= 65 536
    rows: 32 -> 32 both directions, 32 -> 16 forward, 16 -> 32 backward data; round 6: the plain 16 -> 16 forward) and conv_rows_first
    (round 6: 4 / 5 point features -> 16 / 32 channels, forward) are what the heuristic launches for the backbones' first two levels; with
    fv2p_sparse_conv_set_paths(0, 0) the staged kernels take the same launches.  Both settings against the oracle's gather -> mm ->
    scatter loop (spconv_ops.h:260-457) at 1e-4, forward and input gradient, at row counts around the 16-row group, the 64-row tile
    and conv_rows_res's 65 536-row gate (65 537 rows: the staged kernel runs in both settings there); and against each other to
    1e-6 of the output's scale (same k order; the position of a product inside a wave's MFMA chain may differ)."""
    import fv2p_native
    batch = 2
    shape = [5, 12, 12] if n_rows < 100 else [8, 40, 40] if n_rows < 10000 else [12, 96, 96]
    ind, feats, _ = make_input(cin * 1000 + cout + n_rows, batch, shape, n_rows, cin, gpu)
    assert ind.shape[0] == n_rows
    torch.manual_seed(cin + cout)
    conv = spconv.SubMConv3d(cin, cout, 3, padding=1, bias=False, indice_key="k").to(gpu)
    w = conv.weight.detach().cpu().numpy()
    _, pairs, num = oracle.indice_pairs(ind, batch, shape, [3, 3, 3], [1, 1, 1], [1, 1, 1], [1, 1, 1], subm=True)
    ref = oracle.indice_conv(feats, w, pairs, num, n_rows, subm=True).numpy()
    g = np.random.default_rng(7).standard_normal(ref.shape).astype(np.float32)
    din, _ = oracle.indice_conv_backward(feats, w, g, pairs, num, subm=True)
    got = {}
    try:
        for on in (1, 0):
            fv2p_native.call("fv2p_sparse_conv_set_paths", on, on)
            x = spconv.SparseConvTensor(torch.from_numpy(feats).to(gpu).requires_grad_(True), torch.from_numpy(ind).to(gpu), shape, batch)
            y = conv(x)
            y.features.backward(torch.from_numpy(g).to(gpu))
            got[on] = (y.features.detach().cpu().numpy(), x.features.grad.cpu().numpy())
            assert rel_err(got[on][0], ref) < RTOL, ("forward", on)
            assert rel_err(got[on][1], din.numpy()) < RTOL, ("backward data", on)
    finally:
        fv2p_native.call("fv2p_sparse_conv_set_paths", -1, -1)
    assert rel_err(got[1][0], got[0][0]) < 1e-6 and rel_err(got[1][1], got[0][1]) < 1e-6


def test_thin_layer_switch_selects_the_kernels(gpu):
    """The switch is live (not a process-static read of the environment): the conv kernel trace hook is NULL-safe in both settings and
    the two settings' outputs are produced by different kernels - seen as different launch counts of conv_rows_thin in rocprof
    (profiles/r05_*), here as the ABI accepting 1 / 0 / -1 and rejecting anything else."""
    import fv2p_native
    for v in (1, 0, -1):
        fv2p_native.call("fv2p_sparse_conv_set_paths", v, v)
    with pytest.raises(fv2p_native.Fv2pError):
        fv2p_native.call("fv2p_sparse_conv_set_paths", 2, 0)
    fv2p_native.call("fv2p_sparse_conv_set_paths", -1, -1)


@pytest.mark.parametrize("k,s,p", [([3, 3, 3], [2, 2, 2], [1, 1, 1]), ([3, 3, 3], [2, 2, 2], [0, 1, 1]), ([3, 1, 1], [2, 1, 1], [0, 0, 0]),
                                   ([2, 2, 2], [2, 2, 2], [0, 0, 0]), ([3, 3, 3], [1, 1, 1], [1, 1, 1])])
def test_strided_conv_vs_oracle_and_dense(gpu, front_end, k, s, p):
    batch, shape, cin, cout = 2, [9, 16, 14], 16, 32
    ind, feats, x = make_input(11, batch, shape, 500, cin, gpu)
    conv = spconv.SparseConv3d(cin, cout, k, stride=s, padding=p, bias=True).to(gpu)
    x.features.requires_grad_(True)
    y = conv(x)
    w, b = conv.weight.detach().cpu(), conv.bias.detach().cpu()
    outids, pairs, num = oracle.indice_pairs(ind, batch, shape, k, s, p, [1, 1, 1])
    assert np.array_equal(y.indices.cpu().numpy(), outids)
    ref = oracle.indice_conv(feats, w.numpy(), pairs, num, outids.shape[0]).numpy() + b.numpy()
    assert rel_err(y.features.detach().cpu().numpy(), ref) < RTOL
    # dense equivalence: conv3d over the densified input, sampled at the active output sites
    dense_in = torch.zeros((batch, cin, *shape))
    dense_in[ind[:, 0], :, ind[:, 1], ind[:, 2], ind[:, 3]] = torch.from_numpy(feats)
    wd = w.permute(4, 3, 0, 1, 2).contiguous()  # [kz,ky,kx,Cin,Cout] -> [Cout,Cin,kz,ky,kx]
    dense_out = F.conv3d(dense_in, wd, b, stride=s, padding=p)
    assert list(dense_out.shape[2:]) == list(y.spatial_shape)
    samp = dense_out[outids[:, 0], :, outids[:, 1], outids[:, 2], outids[:, 3]].numpy()
    assert rel_err(y.features.detach().cpu().numpy(), samp) < RTOL
    mask = torch.zeros((batch, *y.spatial_shape), dtype=torch.bool)
    mask[outids[:, 0], outids[:, 1], outids[:, 2], outids[:, 3]] = True
    inactive = (dense_out - b.view(1, -1, 1, 1, 1)).permute(0, 2, 3, 4, 1)[~mask]
    assert inactive.abs().max() < 1e-5  # the sparse output set is exactly the reachable set
    assert rel_err(y.dense().detach().cpu().numpy(), (dense_out * mask.unsqueeze(1)).numpy()) < RTOL
    # backward vs oracle
    g = np.random.default_rng(3).standard_normal(ref.shape).astype(np.float32)
    y.features.backward(torch.from_numpy(g).to(gpu))
    din, dw = oracle.indice_conv_backward(feats, w.numpy(), g, pairs, num)
    assert rel_err(x.features.grad.cpu().numpy(), din.numpy()) < RTOL
    assert rel_err(conv.weight.grad.cpu().numpy(), dw.numpy()) < RTOL
    assert rel_err(conv.bias.grad.cpu().numpy(), g.sum(0)) < RTOL


def test_128_channels_with_more_than_27_offsets_vs_oracle(gpu):
    """128 -> 128 with a 4 x 2 x 4 kernel (32 offsets): past the 27 offsets the K-split tile's step list holds, so the auto mode
    takes the LDS-DMA tile on two column halves (conv_rows_dma<128, 4> on grid.y = 2), forward and backward data."""
    batch, shape, cin, cout, k, s, p = 2, [9, 16, 14], 128, 128, [4, 2, 4], [1, 1, 1], [1, 0, 1]
    ind, feats, x = make_input(17, batch, shape, 300, cin, gpu)
    conv = spconv.SparseConv3d(cin, cout, k, stride=s, padding=p, bias=True).to(gpu)
    x.features.requires_grad_(True)
    y = conv(x)
    w, b = conv.weight.detach().cpu().numpy(), conv.bias.detach().cpu().numpy()
    outids, pairs, num = oracle.indice_pairs(ind, batch, shape, k, s, p, [1, 1, 1])
    assert np.array_equal(y.indices.cpu().numpy(), outids) and outids.shape[0] > 128   # more than one 64-row tile
    ref = oracle.indice_conv(feats, w, pairs, num, outids.shape[0]).numpy() + b
    assert rel_err(y.features.detach().cpu().numpy(), ref) < RTOL
    g = np.random.default_rng(3).standard_normal(ref.shape).astype(np.float32)
    y.features.backward(torch.from_numpy(g).to(gpu))
    din, dw = oracle.indice_conv_backward(feats, w, g, pairs, num)
    assert rel_err(x.features.grad.cpu().numpy(), din.numpy()) < RTOL
    assert rel_err(conv.weight.grad.cpu().numpy(), dw.numpy()) < RTOL


def test_subm_conv_equals_masked_dense_conv_and_autograd(gpu):
    batch, shape, cin, cout = 2, [7, 12, 10], 8, 16
    ind, feats, x = make_input(5, batch, shape, 400, cin, gpu)
    conv = spconv.SubMConv3d(cin, cout, 3, padding=1, bias=True, indice_key="s").to(gpu)
    x.features.requires_grad_(True)
    y = conv(x)
    w = conv.weight.detach().cpu().clone().requires_grad_(True)
    fd = torch.from_numpy(feats).clone().requires_grad_(True)
    idx = tuple(torch.from_numpy(ind[:, j]).long() for j in range(4))
    dense_in = torch.zeros((batch, *shape, cin)).index_put(idx, fd).permute(0, 4, 1, 2, 3)
    dense_out = F.conv3d(dense_in, w.permute(4, 3, 0, 1, 2), conv.bias.detach().cpu(), padding=1)
    samp = dense_out[ind[:, 0], :, ind[:, 1], ind[:, 2], ind[:, 3]]
    assert rel_err(y.features.detach().cpu().numpy(), samp.detach().numpy()) < RTOL
    g = torch.from_numpy(np.random.default_rng(9).standard_normal(samp.shape).astype(np.float32))
    samp.backward(g)
    y.features.backward(g.to(gpu))
    assert rel_err(x.features.grad.cpu().numpy(), fd.grad.numpy()) < RTOL
    assert rel_err(conv.weight.grad.cpu().numpy(), w.grad.numpy()) < RTOL


def test_inverse_and_transposed_conv(gpu, front_end):
    batch, shape, c = 2, [8, 12, 12], 16
    ind, feats, x = make_input(21, batch, shape, 350, c, gpu)
    down = spconv.SparseConv3d(c, 32, 3, stride=2, padding=1, bias=False, indice_key="d").to(gpu)
    up = spconv.SparseInverseConv3d(32, c, 3, indice_key="d", bias=False).to(gpu)
    x.features.requires_grad_(True)
    mid = down(x)
    y = up(mid)
    assert torch.equal(y.indices, x.indices) and list(y.spatial_shape) == shape
    outids, pairs, num = oracle.indice_pairs(ind, batch, shape, [3, 3, 3], [2, 2, 2], [1, 1, 1], [1, 1, 1])
    m_ref = oracle.indice_conv(feats, down.weight.detach().cpu().numpy(), pairs, num, outids.shape[0])
    y_ref = oracle.indice_conv(m_ref, up.weight.detach().cpu().numpy(), pairs, num, ind.shape[0], inverse=True)
    assert rel_err(y.features.detach().cpu().numpy(), y_ref.numpy()) < RTOL
    g = np.random.default_rng(1).standard_normal(y_ref.shape).astype(np.float32)
    y.features.backward(torch.from_numpy(g).to(gpu))
    dmid, dw_up = oracle.indice_conv_backward(m_ref, up.weight.detach().cpu().numpy(), g, pairs, num, inverse=True)
    din, dw_dn = oracle.indice_conv_backward(feats, down.weight.detach().cpu().numpy(), dmid.numpy(), pairs, num)
    assert rel_err(up.weight.grad.cpu().numpy(), dw_up.numpy()) < RTOL
    assert rel_err(down.weight.grad.cpu().numpy(), dw_dn.numpy()) < RTOL
    assert rel_err(x.features.grad.cpu().numpy(), din.numpy()) < RTOL
    # transposed conv == conv_transpose3d on the dense tensor
    tconv = spconv.SparseConvTranspose3d(c, 8, 3, stride=2, padding=1, bias=False).to(gpu)
    ind2, feats2, x2 = make_input(22, 1, [4, 6, 6], 60, c, gpu)
    y2 = tconv(x2)
    dense_in = torch.zeros((1, c, 4, 6, 6))
    dense_in[ind2[:, 0], :, ind2[:, 1], ind2[:, 2], ind2[:, 3]] = torch.from_numpy(feats2)
    wt = tconv.weight.detach().cpu().permute(3, 4, 0, 1, 2).contiguous()  # [Cin,Cout,kz,ky,kx]
    dense_out = F.conv_transpose3d(dense_in, wt, stride=2, padding=1)
    oi = y2.indices.cpu().numpy()
    assert list(dense_out.shape[2:]) == list(y2.spatial_shape)
    assert rel_err(y2.features.detach().cpu().numpy(), dense_out[oi[:, 0], :, oi[:, 1], oi[:, 2], oi[:, 3]].numpy()) < RTOL


def test_rulebook_cache_and_sequential_semantics(gpu):
    """indice_key caching (conv.py:150-183), in-place feature mutation by SparseSequential (modules.py:134)."""
    ind, feats, x = make_input(31, 2, [9, 16, 16], 400, 16, gpu)
    net = spconv.SparseSequential(
        spconv.SubMConv3d(16, 16, 3, padding=1, bias=False, indice_key="subm1"), torch.nn.BatchNorm1d(16), torch.nn.ReLU(),
        spconv.SubMConv3d(16, 16, 3, padding=1, bias=False, indice_key="subm1"), torch.nn.BatchNorm1d(16), torch.nn.ReLU(),
        spconv.SparseConv3d(16, 32, 3, stride=2, padding=1, bias=False, indice_key="spconv2"),
    ).to(gpu)
    y = net(x)
    assert set(x.indice_dict.keys()) == {"subm1", "spconv2"} and y.indice_dict is x.indice_dict
    rb = x.indice_dict["subm1"]
    outids, indices, pairs, pair_num, sshape = rb  # the reference's 5-tuple contract (conv.py:180-183)
    assert pairs.shape == (27, 2, ind.shape[0]) and int(pair_num[13]) == ind.shape[0] and list(sshape) == [9, 16, 16]
    assert y.features.shape[1] == 32 and y.dense().shape == (2, 32, 5, 8, 8)
    # the functional API with reference-format pair tensors gives the same result as the module path
    w = net[0].weight
    a = spconv.functional.indice_subm_conv(torch.from_numpy(feats).to(gpu), w, pairs, pair_num, ind.shape[0]) if hasattr(spconv, "functional") else None
    from pcdet.ops.spconv import functional as Fsp
    a = Fsp.indice_subm_conv(torch.from_numpy(feats).to(gpu), w, pairs, pair_num, ind.shape[0])
    b = Fsp.indice_subm_conv(torch.from_numpy(feats).to(gpu), w, rb, pair_num, ind.shape[0])
    assert torch.equal(a, b)
    # fused() folds BN into a biased conv (inference)
    net.eval()
    x1 = spconv.SparseConvTensor(torch.from_numpy(feats).to(gpu), torch.from_numpy(ind).to(gpu), [9, 16, 16], 2)
    x2 = spconv.SparseConvTensor(torch.from_numpy(feats).to(gpu), torch.from_numpy(ind).to(gpu), [9, 16, 16], 2)
    with torch.no_grad():
        r1, r2 = net(x1), net.fused()(x2)
    assert rel_err(r2.features.cpu().numpy(), r1.features.cpu().numpy()) < 1e-4


def test_ext_module_surface_and_foreign_pairs(gpu):
    """sparse_conv_ext keeps the 17 pybind names (all.cc:22-71); pair tensors built elsewhere are accepted."""
    from pcdet.ops.spconv import sparse_conv_ext as ext
    names = ["get_indice_pairs_2d", "get_indice_pairs_3d", "get_indice_pairs_4d", "get_indice_pairs_grid_2d", "get_indice_pairs_grid_3d",
             "indice_conv_fp32", "indice_conv_backward_fp32", "indice_conv_half", "indice_conv_backward_half", "fused_indice_conv_fp32",
             "fused_indice_conv_half", "indice_maxpool_fp32", "indice_maxpool_backward_fp32", "indice_maxpool_half",
             "indice_maxpool_backward_half", "indice_group_fp32", "indice_group_backward_fp32"]
    assert all(hasattr(ext, n) for n in names)
    batch, shape, cin, cout = 1, [6, 10, 10], 16, 16
    ind, feats, _ = make_input(41, batch, shape, 200, cin, gpu)
    outids, pairs, num = oracle.indice_pairs(ind, batch, shape, [3, 3, 3], [2, 2, 2], [1, 1, 1], [1, 1, 1], canonical=False)
    w = torch.randn(3, 3, 3, cin, cout, generator=torch.Generator().manual_seed(0))
    f = torch.from_numpy(feats).to(gpu)
    out = ext.indice_conv_fp32(f, w.to(gpu), torch.from_numpy(pairs).to(gpu), torch.from_numpy(num), outids.shape[0], 0, 0)
    ref = oracle.indice_conv(feats, w.numpy(), pairs, num, outids.shape[0])
    assert rel_err(out.cpu().numpy(), ref.numpy()) < RTOL
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(1))
    din, dw = ext.indice_conv_backward_fp32(f, w.to(gpu), g.to(gpu), torch.from_numpy(pairs).to(gpu), torch.from_numpy(num), 0, 0)
    rdin, rdw = oracle.indice_conv_backward(feats, w.numpy(), g.numpy(), pairs, num)
    assert rel_err(din.cpu().numpy(), rdin.numpy()) < RTOL and rel_err(dw.cpu().numpy(), rdw.numpy()) < RTOL
    bias = torch.randn(cout)
    fo = ext.fused_indice_conv_fp32(f, w.to(gpu), bias.to(gpu), torch.from_numpy(pairs).to(gpu), torch.from_numpy(num), outids.shape[0], 0, 0)
    assert rel_err(fo.cpu().numpy(), (ref + bias).numpy()) < RTOL
    # half entry points compute in fp32 and round once
    oh = ext.indice_conv_half(f.half(), w.half().to(gpu), torch.from_numpy(pairs).to(gpu), torch.from_numpy(num), outids.shape[0], 0, 0)
    assert oh.dtype == torch.half and rel_err(oh.float().cpu().numpy(), ref.numpy()) < 2e-2


def test_maxpool_and_group(gpu):
    batch, shape, c = 2, [8, 12, 12], 16
    ind, feats, x = make_input(51, batch, shape, 500, c, gpu)
    pool = spconv.SparseMaxPool3d(3, stride=2, padding=1)
    x.features.requires_grad_(True)
    y = pool(x)
    outids, pairs, num = oracle.indice_pairs(ind, batch, shape, [3, 3, 3], [2, 2, 2], [1, 1, 1], [1, 1, 1])
    ref = oracle.indice_maxpool(feats, pairs, num, outids.shape[0])
    assert np.array_equal(y.indices.cpu().numpy(), outids)
    assert np.array_equal(y.features.detach().cpu().numpy(), ref)  # pure selection: bit-exact
    assert (ref >= 0).all()  # reference quirk: output starts at zero (pool_ops.h:34)
    g = np.random.default_rng(2).standard_normal(ref.shape).astype(np.float32)
    y.features.backward(torch.from_numpy(g).to(gpu))
    rdin = oracle.indice_maxpool_backward(feats, ref, g, pairs, num)
    assert rel_err(x.features.grad.cpu().numpy(), rdin) < 1e-6
    # group: (N, C) -> (N, K, C)
    _, feats2, x2 = make_input(51, batch, shape, 500, c, gpu)
    grp = spconv.SubMGroup3d(c, 3, indice_key="g")
    x2.features.requires_grad_(True)
    z = grp(x2)
    _, sp, sn = oracle.indice_pairs(ind, batch, shape, [3, 3, 3], [1, 1, 1], [1, 1, 1], [1, 1, 1], subm=True)
    gref = oracle.indice_group(feats2, sp, sn, ind.shape[0])
    assert z.features.shape == (ind.shape[0], 27, c)
    assert np.array_equal(z.features.detach().cpu().numpy(), gref.transpose(1, 0, 2))
    gg = np.random.default_rng(4).standard_normal(z.features.shape).astype(np.float32)
    z.features.backward(torch.from_numpy(gg).to(gpu))
    # d_feat[i] = sum over pairs (i, o, k) of grad[o, k]
    rd = np.zeros_like(feats2)
    for k in range(27):
        n = int(sn[k])
        np.add.at(rd, sp[k, 0, :n], gg[sp[k, 1, :n], k])
    assert rel_err(x2.features.grad.cpu().numpy(), rd) < 1e-5
    sg = spconv.SparseGroup3d(c, 3, stride=2, padding=1)
    z2 = sg(make_input(51, batch, shape, 500, c, gpu)[2])
    assert np.array_equal(z2.features.cpu().numpy(), oracle.indice_group(feats, pairs, num, outids.shape[0]).transpose(1, 0, 2))


def test_empty_and_tiny_inputs(gpu):
    conv = spconv.SubMConv3d(16, 16, 3, padding=1, bias=False).to(gpu)
    x = spconv.SparseConvTensor(torch.zeros((0, 16), device=gpu), torch.zeros((0, 4), dtype=torch.int32, device=gpu), [4, 4, 4], 1)
    assert conv(x).features.shape == (0, 16)
    x = spconv.SparseConvTensor(torch.ones((1, 16), device=gpu), torch.zeros((1, 4), dtype=torch.int32, device=gpu), [4, 4, 4], 1)
    y = conv(x)
    assert rel_err(y.features.detach().cpu().numpy(), conv.weight[1, 1, 1].sum(0, keepdim=True).detach().cpu().numpy()) < RTOL
    with pytest.raises(Exception):  # CPU tensors fail loudly: there is no CPU path
        conv.cpu()(spconv.SparseConvTensor(torch.ones((1, 16)), torch.zeros((1, 4), dtype=torch.int32), [4, 4, 4], 1))


def test_rulebook_prefetch_recipe_matches_inline_build_and_ignores_stale_geometry(gpu):
    """spconv.rulebook_recipe / build_rulebooks / attach_rulebooks (input-pipeline prefetch): a pass that finds every
    indice_key prefetched gives bit-identical features and indices to the pass that builds its rulebooks in line, on
    new coordinates; an attached rulebook with another geometry is ignored (rebuilt), not used."""
    batch, shape = 2, [17, 40, 36]

    def net(pad=1):
        torch.manual_seed(1)
        return spconv.SparseSequential(
            spconv.SubMConv3d(8, 16, 3, padding=1, bias=False, indice_key="subm1"),
            spconv.SparseConv3d(16, 32, 3, stride=2, padding=pad, bias=False, indice_key="spconv2"),
            spconv.SubMConv3d(32, 32, 3, padding=1, bias=False, indice_key="subm2"),
            spconv.SparseConv3d(32, 32, (3, 1, 1), stride=(2, 1, 1), padding=0, bias=False, indice_key="down"),
            spconv.SparseInverseConv3d(32, 16, (3, 1, 1), indice_key="down", bias=False)).to(gpu)

    model = net()
    ind0, f0, x0 = make_input(11, batch, shape, 1500, 8, gpu)
    y0 = model(x0)
    recipe = spconv.rulebook_recipe(y0.indice_dict, x0.indices)
    assert [r[0] for r in recipe] == ["subm1", "spconv2", "subm2", "down"] and [r[1] for r in recipe] == [None, None, "spconv2", "spconv2"]
    ind1, f1, x1 = make_input(12, batch, shape, 1700, 8, gpu)
    ref = model(x1)
    coords = torch.from_numpy(ind1).to(gpu)
    built = spconv.build_rulebooks(recipe, coords, batch)
    spconv.attach_rulebooks(coords, built)
    x2 = spconv.SparseConvTensor(torch.from_numpy(f1).to(gpu), coords, shape, batch)
    assert set(x2.indice_dict) == {"subm1", "spconv2", "subm2", "down"}
    calls = []
    orig = ops.build_rulebook
    ops.build_rulebook = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    try:
        out = model(x2)
        assert calls == []                                        # every key was a cache hit
        assert torch.equal(out.features, ref.features) and torch.equal(out.indices, ref.indices)
        # stale geometry: same keys, but the model's strided conv now has another padding -> rebuilt, result = inline
        model2 = net(pad=0)
        x3 = spconv.SparseConvTensor(torch.from_numpy(f1).to(gpu), coords, shape, batch)
        out3 = model2(x3)
        assert len(calls) >= 1
    finally:
        ops.build_rulebook = orig
    x4 = spconv.SparseConvTensor(torch.from_numpy(f1).to(gpu), torch.from_numpy(ind1).to(gpu), shape, batch)
    ref3 = model2(x4)
    assert torch.equal(out3.indices, ref3.indices) and torch.equal(out3.features, ref3.features)


@pytest.mark.parametrize("staged", [False, True], ids=["lds-dma", "register-staged"])
@pytest.mark.parametrize("cin,cout", [(16, 16), (32, 64), (64, 64), (5, 16), (128, 64), (64, 128), (128, 128), (160, 144)])
def test_weight_gradient_from_pair_lists_vs_oracle(gpu, front_end, cin, cout, staged):
    """fv2p_sparse_conv_wgrad_pairs (work split by the rulebook's reference-format pair lists, used once
    indice_pairs / indice_pair_num are materialised, e.g. by the rulebook prefetch): dW of a submanifold conv, a strided
    conv and its inverse conv against the oracle's gather -> mm loop (spconv_ops.h:403-455 restated)."""
    batch, shape = 2, [9, 20, 18]
    ind, feats, x = make_input(cin * 3 + cout, batch, shape, 1300, cin, gpu)
    torch.manual_seed(0)
    net = spconv.SparseSequential(
        spconv.SubMConv3d(cin, cout, 3, padding=1, bias=False, indice_key="s"),
        spconv.SparseConv3d(cout, cout, 3, stride=2, padding=1, bias=False, indice_key="d"),
        spconv.SparseInverseConv3d(cout, cin, 3, indice_key="d", bias=False)).to(gpu)
    with torch.no_grad():
        net(x)                                       # fills x.indice_dict
    for i, rb in enumerate(x.indice_dict.values()):
        if i == 0:
            rb.wgrad_pairs()                         # compacted lists without the -1 padding pass
        else:
            rb.indice_pairs, rb.indice_pair_num      # reference-format lists; either way the backward takes the pair-list kernel
        assert rb._wpairs is not None and rb._num is not None
    import fv2p_native
    x.features.requires_grad_(True)
    try:
        if staged:   # forcing a conv variant also selects the register-staged pair-split kernel (64/128 channels: LDS-DMA otherwise)
            fv2p_native.call("fv2p_sparse_conv_set_impl", 3)
        y = net(x)
        g = np.random.default_rng(5).standard_normal(tuple(y.features.shape)).astype(np.float32)
        y.features.backward(torch.from_numpy(g).to(gpu))
    finally:
        fv2p_native.call("fv2p_sparse_conv_set_impl", 0)
    # oracle chain
    w = [m.weight.detach().cpu().numpy() for m in net]
    _, p_s, n_s = oracle.indice_pairs(ind, batch, shape, [3, 3, 3], [1, 1, 1], [1, 1, 1], [1, 1, 1], subm=True)
    out_d, p_d, n_d = oracle.indice_pairs(ind, batch, shape, [3, 3, 3], [2, 2, 2], [1, 1, 1], [1, 1, 1])
    f1 = oracle.indice_conv(feats, w[0], p_s, n_s, ind.shape[0], subm=True).numpy()
    f2 = oracle.indice_conv(f1, w[1], p_d, n_d, out_d.shape[0]).numpy()
    d2, dw2 = oracle.indice_conv_backward(f2, w[2], g, p_d, n_d, inverse=True)
    d1, dw1 = oracle.indice_conv_backward(f1, w[1], d2.numpy(), p_d, n_d)
    d0, dw0 = oracle.indice_conv_backward(feats, w[0], d1.numpy(), p_s, n_s, subm=True)
    for m, ref in zip(net, (dw0, dw1, dw2)):
        assert rel_err(m.weight.grad.cpu().numpy(), ref.numpy()) < RTOL
    assert rel_err(x.features.grad.cpu().numpy(), d0.numpy()) < RTOL


@pytest.mark.parametrize("ndim", [3, 2])
def test_dense_scatter_equals_reference_expression_and_gradient(gpu, ndim):
    """SparseConvTensor.dense() on the GPU (fv2p_sparse_to_dense / fv2p_dense_to_sparse) against the reference's
    expression zeros -> scatter_nd -> permute (structure.py:5-18, 57-66), both layouts, values bit-exact, gradient
    = the rows of the dense gradient."""
    batch, c = 3, 24
    shape = [5, 12, 10] if ndim == 3 else [12, 10]
    rng = np.random.default_rng(0)
    cells = rng.permutation(batch * int(np.prod(shape)))[:300]
    ind = np.stack(np.unravel_index(cells, [batch] + shape), 1).astype(np.int32)
    feats = rng.standard_normal((300, c)).astype(np.float32)
    for channels_first in (True, False):
        f = torch.from_numpy(feats).to(gpu).requires_grad_(True)
        x = spconv.SparseConvTensor(f, torch.from_numpy(ind).to(gpu), shape, batch)
        d = x.dense(channels_first)
        ref = spconv.scatter_nd(torch.from_numpy(ind).long(), torch.from_numpy(feats), [batch] + shape + [c])
        if channels_first:
            perm = list(range(0, ndim + 1))
            perm.insert(1, ndim + 1)
            ref = ref.permute(*perm).contiguous()
        assert d.shape == ref.shape and torch.equal(d.cpu(), ref)
        g = torch.from_numpy(rng.standard_normal(tuple(ref.shape)).astype(np.float32))
        d.backward(g.to(gpu))
        gl = g if not channels_first else g.permute(*([0] + list(range(2, ndim + 2)) + [1]))
        want = gl[tuple(torch.from_numpy(ind[:, i]).long() for i in range(ndim + 1))]
        assert torch.equal(f.grad.cpu(), want)


def test_deferred_weight_gradient_join_gives_the_same_gradients(gpu):
    """spconv.defer_weight_gradients (compiled binding): every conv's dW runs on the side stream and is joined once at
    the end of backward.  Gradients are bit-identical to the per-layer join, over several iterations with the training
    stream's allocator recycling blocks in between; a conv applied twice (second use: plain weight, immediate join) and a
    conv left out of the pass are handled."""
    import fv2p_native
    if fv2p_native.torch_ext() is None:
        pytest.skip("compiled binding not built")
    batch, shape = 2, [9, 40, 36]

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            bn = lambda c: torch.nn.BatchNorm1d(c, eps=1e-3, momentum=0.01)
            self.a = spconv.SparseSequential(spconv.SubMConv3d(16, 32, 3, padding=1, bias=False, indice_key="s1"), bn(32), torch.nn.ReLU())
            self.b = spconv.SparseSequential(spconv.SubMConv3d(32, 32, 3, padding=1, bias=False, indice_key="s1"), bn(32), torch.nn.ReLU())
            self.c = spconv.SparseSequential(spconv.SparseConv3d(32, 64, 3, stride=2, padding=1, bias=False, indice_key="d"), bn(64), torch.nn.ReLU())
            self.unused = spconv.SubMConv3d(64, 64, 3, padding=1, bias=False, indice_key="s2")
            self.defer = False

        def forward(self, x):
            if self.defer:
                spconv.defer_weight_gradients(self)
            return self.c(self.b(self.b(self.a(x))))      # self.b twice: shared weight

    torch.manual_seed(0)
    net = Net().to(gpu)
    results = {}
    for defer in (False, True):
        net.defer = defer
        grads = []
        for it in range(4):
            ind, feats, x = make_input(100 + it, batch, shape, 3000, 16, gpu)
            x.features.requires_grad_(True)
            net.zero_grad(set_to_none=True)
            y = net(x)
            junk = [torch.empty(int(n), device=gpu) for n in (1e6, 3e5, 2e6)]   # churn the allocator around backward
            y.features.square().sum().backward()
            del junk
            junk = [torch.zeros(int(n), device=gpu) for n in (2e6, 1e6)]
            grads.append([p.grad.clone() if p.grad is not None else None for p in net.parameters()] + [x.features.grad.clone()])
            del junk
        torch.cuda.synchronize()
        results[defer] = grads
    assert net.unused.weight.grad is None
    for ga, gb in zip(results[False], results[True]):
        for a, b in zip(ga, gb):
            assert (a is None) == (b is None)
            if a is not None:
                assert torch.equal(a, b)


@pytest.mark.parametrize("impl", [0, 1, 2, 3, 4])
def test_conv_epilogue_statistics_equal_the_column_sums(gpu, impl):
    """fv2p_sparse_conv_rows_stats (C ABI): dst is bit-identical to fv2p_sparse_conv_rows and the slots of `stats` add up to
    the fp64 column sums / sums of squares of dst — for every kernel variant, with and without a bias, rows not a multiple
    of the 64-row tile, scalar (cin 4, 24) and split (cin 160) shapes; a second call keeps adding (caller zero-fills)."""
    import fv2p_native
    slots = int(fv2p_native.lib().fv2p_sparse_conv_stat_slots())
    batch, shape = 2, [9, 20, 18]
    try:
        fv2p_native.call("fv2p_sparse_conv_set_impl", impl)
        for cin, cout, subm in [(4, 16, True), (16, 16, True), (32, 64, False), (64, 64, True), (64, 128, True), (128, 128, True), (24, 40, False), (160, 144, True)]:
            ind, feats, x = make_input(cin + cout, batch, shape, 1100, cin, gpu)
            rb = ops.build_rulebook(x.indices, batch, shape, 3, 1 if subm else 2, 1, 1, 0, subm)
            n_out = rb.outids.shape[0]
            tab, flip = rb.out_table()
            rng = np.random.default_rng(cin)
            w = torch.from_numpy(rng.standard_normal((27, cin, cout)).astype(np.float32) * 0.1).to(gpu)
            for bias in (None, torch.from_numpy(rng.standard_normal(cout).astype(np.float32)).to(gpu)):
                ref = torch.empty((n_out, cout), device=gpu)
                fv2p_native.call("fv2p_sparse_conv_rows", x.features, x.features.shape[0], cin, w, 27, tab, n_out, cout, int(flip), 0, bias, ref,
                                 fv2p_native.stream())
                dst = torch.empty_like(ref)
                stats = torch.zeros((slots, 2, cout), dtype=torch.float64, device=gpu)
                for rep in (1, 2):
                    fv2p_native.call("fv2p_sparse_conv_rows_stats", x.features, x.features.shape[0], cin, w, 27, tab, n_out, cout, int(flip), 0, bias,
                                     dst, stats, fv2p_native.stream())
                    assert torch.equal(dst, ref), (impl, cin, cout)
                    if rep == 2 and not (cin <= 128 and impl != 2):
                        break    # the reduce-pass fallback stores its partials instead of adding: one call per zero-fill
                    tot = stats.sum(0).cpu().numpy()
                    d64 = ref.double().cpu().numpy()
                    want = np.stack([d64.sum(0), (d64 * d64).sum(0)]) * rep
                    assert np.allclose(tot, want, rtol=1e-11, atol=1e-9), (impl, cin, cout, rep)
    finally:
        fv2p_native.call("fv2p_sparse_conv_set_impl", 0)


def test_batchnorm_sums_from_conv_epilogues_match_the_separate_passes(gpu):
    """Compiled binding: in a conv -> BN -> ReLU chain the forward column sums come from the conv's epilogue and the
    BatchNorm backward sums from the epilogue of the next layer's backward-data conv (two alternating slot buffers per
    stream and direction).  Features, running statistics and all gradients equal the path where BatchNorm reduces by
    itself (fp64 sums in another order: 1e-5), over several iterations; a BatchNorm whose output feeds two consumers
    (its dy is a sum) falls back by itself."""
    import fv2p_native
    ext = fv2p_native.torch_ext()
    if ext is None:
        pytest.skip("compiled binding not built")
    batch, shape = 2, [9, 40, 36]

    def block(cin, cout, key, **kw):
        conv = spconv.SubMConv3d(cin, cout, 3, padding=1, bias=False, indice_key=key) if not kw else \
            spconv.SparseConv3d(cin, cout, 3, bias=False, indice_key=key, **kw)
        return spconv.SparseSequential(conv, torch.nn.BatchNorm1d(cout, eps=1e-3, momentum=0.01), torch.nn.ReLU())

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a, self.b = block(16, 32, "s1"), block(32, 32, "s1")
            self.c = block(32, 64, "d", stride=2, padding=1)
            self.d, self.e = block(64, 64, "s2"), block(64, 160, "s2")      # 160 output channels: dX sums by the fallback pass
            self.f = block(160, 64, "s2")
            self.side = block(32, 32, "s1")

        def forward(self, x):
            xb = self.b(self.a(x))
            y = self.f(self.e(self.d(self.c(xb))))
            z = self.side(xb)                                              # xb feeds two convs: BatchNorm b's dy is a sum
            return y.features.square().sum() + z.features.square().sum()

    results = {}
    try:
        for mode in (True, False):
            ext.set_bn_epilogue(mode)
            torch.manual_seed(0)
            net = Net().to(gpu)
            outs = []
            for it in range(3):
                ind, feats, x = make_input(200 + it, batch, shape, 3000, 16, gpu)
                x.features.requires_grad_(True)
                net.zero_grad(set_to_none=True)
                loss = net(x)
                loss.backward()
                outs.append([loss.detach().clone(), x.features.grad.clone()] + [p.grad.clone() for p in net.parameters()]
                            + [b.clone() for b in net.buffers() if b.dtype == torch.float32])
            results[mode] = outs
    finally:
        ext.set_bn_epilogue(True)
    for it, (oa, ob) in enumerate(zip(results[True], results[False])):
        for j, (a, b) in enumerate(zip(oa, ob)):
            err = float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))
            assert err < 1e-5, (it, j, tuple(a.shape), err)


@pytest.mark.parametrize("impl", [0, 4])
def test_backward_data_conv_leaves_the_batchnorm_backward_sums(gpu, impl):
    """fv2p_sparse_conv_rows_bnbwd (C ABI): dst equals the plain backward-data conv bit for bit; the slots add up to
    sum dz and sum dz * xhat (dz = dst * [y > 0]) computed in float64 from the same fp32 xhat — in the epilogue
    (c_src <= 128) and by the pass after the conv (c_src = 160); on the default kernels and on the pair-compacted tile."""
    import fv2p_native
    slots = int(fv2p_native.lib().fv2p_sparse_conv_stat_slots())
    batch, shape = 2, [9, 20, 18]
    fv2p_native.call("fv2p_sparse_conv_set_impl", impl)
    try:
        _bnbwd_cases(gpu, slots, batch, shape)
    finally:
        fv2p_native.call("fv2p_sparse_conv_set_impl", 0)


def _bnbwd_cases(gpu, slots, batch, shape):
    import fv2p_native
    for cin, cout in [(16, 32), (64, 64), (128, 128), (64, 128), (32, 160), (160, 64), (24, 40)]:     # conv cin -> cout; its dX has c_src = cout, c_dst = cin
        ind, feats, x = make_input(cin * 3 + cout, batch, shape, 1100, cin, gpu)
        rb = ops.build_rulebook(x.indices, batch, shape, 3, 1, 1, 1, 0, True)
        n = x.features.shape[0]
        tab, flip = rb.in_table()
        rng = np.random.default_rng(cout)
        w = torch.from_numpy(rng.standard_normal((27, cin, cout)).astype(np.float32) * 0.1).to(gpu)
        g = torch.from_numpy(rng.standard_normal((n, cout)).astype(np.float32)).to(gpu)
        bn_x = torch.from_numpy(rng.standard_normal((n, cin)).astype(np.float32) * 2 + 1).to(gpu)
        mean = torch.from_numpy(rng.uniform(0.5, 1.5, cin).astype(np.float32)).to(gpu)
        invstd = torch.from_numpy(rng.uniform(0.3, 0.8, cin).astype(np.float32)).to(gpu)
        gamma = torch.from_numpy(rng.uniform(0.5, 1.5, cin).astype(np.float32)).to(gpu)
        beta = torch.from_numpy(rng.uniform(-0.5, 0.5, cin).astype(np.float32)).to(gpu)
        ref = torch.empty((n, cin), device=gpu)
        fv2p_native.call("fv2p_sparse_conv_rows", g, n, cout, w, 27, tab, n, cin, int(flip), 1, None, ref, fv2p_native.stream())
        for relu in (1, 0):
            dst = torch.empty_like(ref)
            stats = torch.zeros((slots, 2, cin), dtype=torch.float64, device=gpu)
            fv2p_native.call("fv2p_sparse_conv_rows_bnbwd", g, n, cout, w, 27, tab, n, cin, int(flip), 1, dst, bn_x, mean, invstd, gamma, beta, relu,
                             stats, None, fv2p_native.stream())
            assert torch.equal(dst, ref), (cin, cout)
            xhat = (bn_x - mean) * invstd                       # fp32, as the kernel
            y = xhat * gamma + beta
            dz = torch.where(y > 0, ref, torch.zeros_like(ref)) if relu else ref
            want = torch.stack([dz.double().sum(0), (dz.double() * xhat.double()).sum(0)]).cpu().numpy()
            assert np.allclose(stats.sum(0).cpu().numpy(), want, rtol=1e-9, atol=1e-7), (cin, cout, relu)


def test_backward_data_of_strided_conv_with_parity_ordered_tiles(gpu):
    """fv2p_rulebook_class_perm + fv2p_sparse_conv_rows_perm / _bnbwd(perm): the permutation is a stable grouping of
    the input rows by (coordinate + padding) mod stride, and the backward-data conv that takes it (tiles visit only the
    offsets their rows use) returns the rows and the BatchNorm sums of the launch in plain row order — bit-identical where
    both launches run the same kernel family; with 64 source channels and whole 64-column blocks the plain launch is the
    pair-compacted K-split tile and the permuted one the offset-skipping tile: two fixed summation orders, 2e-6 apart."""
    import fv2p_native
    slots = int(fv2p_native.lib().fv2p_sparse_conv_stat_slots())
    batch, shape = 2, [11, 40, 36]
    for cin, cout, stride, pad in [(32, 64, (2, 2, 2), (1, 1, 1)), (16, 32, (2, 2, 2), (0, 1, 1)), (64, 64, (2, 1, 1), (0, 0, 0)), (64, 128, (2, 2, 2), (1, 1, 1))]:
        ksize = (3, 1, 1) if stride == (2, 1, 1) else (3, 3, 3)
        kvol = int(np.prod(ksize))
        ind, feats, x = make_input(cin + cout, batch, shape, 5000, cin, gpu)
        rb = ops.build_rulebook(x.indices, batch, shape, ksize, stride, pad, 1, 0, False)
        n, n_out = x.features.shape[0], rb.outids.shape[0]
        perm = torch.empty(n, dtype=torch.int32, device=gpu)
        arr = lambda v: (ctypes.c_int * 3)(*v)
        ws = fv2p_native.workspace(int(fv2p_native.lib().fv2p_rulebook_class_perm_ws_bytes(n)), x.indices.device)
        fv2p_native.call("fv2p_rulebook_class_perm", x.indices, n, arr(stride), arr(pad), perm, ws, ws.numel(), fv2p_native.stream())
        cls = ((x.indices[:, 1:].cpu().numpy() + np.array(pad)) % np.array(stride)) @ np.array([stride[1] * stride[2], stride[2], 1])
        want = np.argsort(cls, kind="stable")
        assert np.array_equal(perm.cpu().numpy(), want)
        tab, flip = rb.in_table()
        rng = np.random.default_rng(cout)
        w = torch.from_numpy(rng.standard_normal((kvol, cin, cout)).astype(np.float32) * 0.1).to(gpu)
        g = torch.from_numpy(rng.standard_normal((n_out, cout)).astype(np.float32)).to(gpu)
        ref = torch.empty((n, cin), device=gpu)
        fv2p_native.call("fv2p_sparse_conv_rows", g, n_out, cout, w, kvol, tab, n, cin, int(flip), 1, None, ref, fv2p_native.stream())
        dst = torch.empty_like(ref)
        fv2p_native.call("fv2p_sparse_conv_rows_perm", g, n_out, cout, w, kvol, tab, n, cin, int(flip), 1, None, dst, perm, fv2p_native.stream())
        mixed = cout == 64 and cin % 64 == 0
        close = lambda a, b: float((a - b).abs().max() / b.abs().max()) < 2e-6
        assert close(dst, ref) if mixed else torch.equal(dst, ref), (cin, cout, stride)
        bn_x = torch.from_numpy(rng.standard_normal((n, cin)).astype(np.float32) * 2 + 1).to(gpu)
        par = [torch.from_numpy(rng.uniform(0.3, 1.5, cin).astype(np.float32)).to(gpu) for _ in range(4)]
        outs = []
        for p in (None, perm):
            dst = torch.empty_like(ref)
            stats = torch.zeros((slots, 2, cin), dtype=torch.float64, device=gpu)
            fv2p_native.call("fv2p_sparse_conv_rows_bnbwd", g, n_out, cout, w, kvol, tab, n, cin, int(flip), 1, dst, bn_x, par[0], par[1], par[2], par[3], 1,
                             stats, p, fv2p_native.stream())
            assert close(dst, ref) if (mixed and p is not None) else torch.equal(dst, ref)
            outs.append(stats.sum(0).cpu().numpy())
        assert np.allclose(outs[0], outs[1], rtol=1e-5 if mixed else 1e-11, atol=1e-3 if mixed else 1e-9)


def test_a_hook_on_a_conv_sees_the_convs_own_output(gpu):
    """SparseSequential offers conv -> BatchNorm1d -> ReLU to the conv as one fused call; a forward hook on the conv (feature taps,
    the roofline probe) must still see what the reference's hook sees: the conv output before BatchNorm / ReLU."""
    ind, feats, x = make_input(9, 2, [9, 20, 18], 900, 16, gpu)
    seq = spconv.SparseSequential(spconv.SubMConv3d(16, 32, 3, padding=1, bias=False, indice_key="s"), nn.BatchNorm1d(32), nn.ReLU()).to(gpu)
    plain = seq(x).features.clone()
    seen = []
    h = list(seq.children())[0].register_forward_hook(lambda m, i, o: seen.append(o.features.clone()))
    hooked = seq(x).features.clone()
    h.remove()
    assert float((hooked - plain).abs().max()) < 1e-5 * float(plain.abs().max())       # same result either way
    assert float(seen[0].min()) < 0 and not torch.equal(seen[0], hooked)             # ... and the hook saw pre-BN / pre-ReLU values


def _plan_of(tab, level_tiles):
    """Host view of the plan behind a table (include/fv2p_ops.h: [magic, levels, per level T + 1 bounds])."""
    kvol, n = tab.shape
    flat = torch.empty(0, dtype=torch.int32, device=tab.device).set_(tab.untyped_storage(), tab.storage_offset() + kvol * n,
                                                                      (tab.untyped_storage().nbytes() // 4 - tab.storage_offset() - kvol * n,))
    plan = flat.cpu().numpy()
    assert plan[0] == 0x706c616e
    off, out = 2, {}
    for lvl in range(int(plan[1])):
        t = (384 if lvl & 1 else 256) << (lvl >> 1)
        out[t] = plan[off:off + t + 1]
        off += t + 1
    return out[level_tiles] if level_tiles else out


@pytest.mark.parametrize("cin,cout,subm", [(64, 64, True), (128, 128, True), (64, 128, False), (128, 128, False)])
def test_tiling_plan_changes_no_bit(gpu, cin, cout, subm):
    """fv2p_conv_plan_build + FV2P_TAB_PLANNED: the cost-balanced tiling is a pure scheduling change — forward, backward-data
    (flipped table for submanifold layers) are bit for bit those of the equal-row tiling, the BatchNorm sums of the epilogue
    (fp64 atomics) equal to 1e-12; the plan's bounds are monotone, cover [0, n) and every range's cost is within one
    row's cost of total / T.  Clustered cloud: dense blobs beside isolated cells, so equal rows are not equal work."""
    import fv2p_native
    slots = int(fv2p_native.lib().fv2p_sparse_conv_stat_slots())
    batch, shape = 2, [21, 60, 56]
    rng = np.random.default_rng(cin + cout + subm)
    cells = set()
    for b in range(batch):
        for _ in range(14):   # blobs
            c = rng.integers([2, 4, 4], [19, 56, 52])
            pts = np.unique(np.clip(np.round(c + rng.standard_normal((700, 3)) * [1.2, 2.5, 2.5]).astype(int), 0, np.array(shape) - 1), axis=0)
            cells.update((b, *p) for p in pts.tolist())
        lone = rng.integers(0, shape, (2500, 3))
        cells.update((b, *p) for p in lone.tolist())
    ind = np.array(sorted(cells), np.int32)
    ind = ind[rng.permutation(ind.shape[0])]
    x = torch.from_numpy(rng.standard_normal((ind.shape[0], cin)).astype(np.float32)).to(gpu)
    indices = torch.from_numpy(ind).to(gpu)
    rb = ops.build_rulebook(indices, batch, shape, 3, 1 if subm else 2, 1, 1, 0, subm)
    n_out = rb.outids.shape[0]
    w = torch.from_numpy(rng.standard_normal((27, cin, cout)).astype(np.float32) * 0.1).to(gpu)
    g = torch.from_numpy(rng.standard_normal((n_out, cout)).astype(np.float32)).to(gpu)
    bias = torch.from_numpy(rng.standard_normal(cout).astype(np.float32)).to(gpu)

    def plan(tab):   # through the C ABI: the Python layer plans submanifold tables only, and from their second conv on (ops.Rulebook._plan)
        kv, nn_ = tab.shape
        ws = fv2p_native.workspace(int(fv2p_native.lib().fv2p_conv_plan_ws_bytes(nn_)), tab.device)
        fv2p_native.call("fv2p_conv_plan_build", tab, kv, nn_, ws, ws.numel(), fv2p_native.stream())

    def run(planned):
        (tab_f, flag_f), (tab_b, flag_b) = rb.out_table(), rb.in_table()
        assert not (flag_f | flag_b) & ops.TAB_PLANNED
        if planned:
            plan(tab_f)
            if tab_b.data_ptr() != tab_f.data_ptr():
                plan(tab_b)
            flag_f, flag_b = flag_f | ops.TAB_PLANNED, flag_b | ops.TAB_PLANNED
        y = torch.empty((n_out, cout), device=gpu)
        stats = torch.zeros((slots, 2, cout), dtype=torch.float64, device=gpu)
        fv2p_native.call("fv2p_sparse_conv_rows_stats", x, x.shape[0], cin, w, 27, tab_f, n_out, cout, int(flag_f), 0, bias, y, stats, fv2p_native.stream())
        dx = torch.empty((x.shape[0], cin), device=gpu)
        fv2p_native.call("fv2p_sparse_conv_rows", g, n_out, cout, w, 27, tab_b, x.shape[0], cin, int(flag_b), 1, None, dx, fv2p_native.stream())
        return y, stats.sum(0), dx

    plain = run(False)
    planned = run(True)
    assert torch.equal(plain[0], planned[0]) and torch.equal(plain[2], planned[2])
    # the epilogue's BatchNorm sums are fp64 atomics into slots chosen by workgroup index: same addends, another order
    assert float((plain[1] - planned[1]).abs().max()) <= 1e-12 * float(plain[1].abs().max())
    # the forward result against the oracle once (the plain tiling is held to it everywhere else)
    _, pairs, num = oracle.indice_pairs(ind, batch, shape, [3, 3, 3], [1, 1, 1] if subm else [2, 2, 2], [1, 1, 1], [1, 1, 1], subm=subm)
    ref = oracle.indice_conv(x.cpu().numpy(), w.cpu().numpy(), pairs, num, n_out, subm=subm).numpy() + bias.cpu().numpy()
    assert rel_err(planned[0].cpu().numpy(), ref) < RTOL
    # structure of the plan behind the forward table
    tab, _ = rb.out_table()
    act = tab.cpu().numpy() >= 0
    cost = np.maximum(act.sum(0), 8)
    n = tab.shape[1]
    csum = np.concatenate([np.zeros((act.shape[0], 1), np.int64), np.cumsum(act, 1)], 1)
    exact_levels = 0
    for tiles, bounds in _plan_of(tab, None).items():
        assert bounds[0] == 0 and bounds[-1] == n and (np.diff(bounds) >= 0).all()
        rows = np.diff(bounds)
        groups = np.ceil((csum[:, bounds[1:]] - csum[:, bounds[:-1]]) / 16).sum(0)
        per = np.add.reduceat(np.concatenate([cost, [0]]), np.minimum(bounds[:-1], cost.size))
        per[rows == 0] = 0
        assert per.sum() == cost.sum()
        if rows.max() <= 64 and groups.max() <= 72 and (rows[rows > 0].min() < rows.max()):
            # exact plan (n <= 32767): greedy runs under one budget of MFMA row groups — every tile but the last of the chain is
            # maximal: one more row would exceed the budget its level chose, or the 64-row cap
            exact_levels += 1
            budget = next(g for g in (28, 30, 32, 34, 36, 38, 40, 42, 44, 46, 48, 52, 56, 60, 64, 72) if groups.max() <= g)
            live = np.nonzero(rows)[0]
            for t in live[:-1]:
                if rows[t] < 64:
                    more = np.ceil((csum[:, bounds[t + 1] + 1] - csum[:, bounds[t]]) / 16).sum()
                    assert more > budget or rows[t] == 1, (tiles, t, more, budget)
        else:   # equal-cost plan
            assert per.max() <= cost.sum() / tiles + cost.max() + 1, (tiles, per.max(), cost.sum() / tiles)
    assert exact_levels > 0 or n > 32767 or n < 1024


def test_python_layer_plans_submanifold_tables_from_the_third_forward_conv(gpu):
    """ops.Rulebook._plan: no plan for strided rulebooks (two convs per table cannot repay 55 - 70 us), none for the first two forward
    convs on a submanifold table (the plain backbone's two per table never repay one), a plan from the third forward request on (the
    residual blocks' four + four); backward convs use a plan that is there but never cause one; build_plan() (input pipelines)
    builds it at once; other channel counts never."""
    ind, feats, x = make_input(5, 2, [9, 20, 18], 1500, 64, gpu)
    sub = ops.build_rulebook(x.indices, 2, [9, 20, 18], 3, 1, 1, 1, 0, True)
    strided = ops.build_rulebook(x.indices, 2, [9, 20, 18], 3, 2, 1, 1, 0, False)
    for _ in range(4):
        assert not strided.out_table(64)[1] & ops.TAB_PLANNED and not strided.in_table(128)[1] & ops.TAB_PLANNED
    assert not sub.out_table(32)[1] & ops.TAB_PLANNED
    assert not sub.out_table(64)[1] & ops.TAB_PLANNED            # first forward request
    for _ in range(4):
        assert not sub.in_table(64)[1] & ops.TAB_PLANNED         # backward requests do not count
    assert not sub.out_table(64)[1] & ops.TAB_PLANNED            # second
    assert sub.out_table(64)[1] & ops.TAB_PLANNED                # third: built
    assert sub.in_table(64)[1] & ops.TAB_PLANNED                 # same table (submanifold symmetry): the backward convs get it too
    assert sub.out_table(32)[1] & ops.TAB_PLANNED                # every later call carries the flag, kernels without plan support ignore it
    fresh = ops.build_rulebook(x.indices, 2, [9, 20, 18], 3, 1, 1, 1, 0, True)
    fresh.build_plan()
    assert fresh.out_table()[1] & ops.TAB_PLANNED
