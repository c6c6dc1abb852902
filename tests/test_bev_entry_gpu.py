"""The first BEV convolution over the sparse rows (pcdet.ops.spconv.bev_entry, csrc/bev_entry.hip + the fused conv kernels) against
float64.

Reference: F.conv2d in float64 on the CPU over the densified input (tests/bev_entry_cases.py); dX is the gradient at the active rows, dW
by autograd, one random upstream gradient.  Bound, per tensor: E = max |torch's own fp32 dense() + F.conv2d path on the GPU - float64|
is measured first and the op may be off by 2 E + 1e-6 (the convention of tests/test_anchor_head_gpu.py: the bound comes from the fp32
reference, never from the kernels under test).  Every E and every error of the op is printed before it is asserted.

The kernel cases call the op with tau = 1 (the sparse route whatever the fill: several of them are small and therefore full); the
routing tests use the default threshold.

dW comes from fv2p_sparse_conv_wgrad_pairs_fine (16-pair fp32 chains folded in float64): with the plain pair-split kernel, which adds a
chunk's up to 256 pairs in one fp32 FMA chain, dW of the 40 x 36 case (150 pairs per offset) was off by 4.3e-05 against a bound of
2.8e-05; with the fine form it is off by 6.8e-06 (torch's own path: 1.2e-05)."""
import copy
import functools

import pytest
import torch

import pcdet.ops.spconv as spconv
from fv2p_harness import fv2p_model as fm
from pcdet.ops.spconv import bev_entry as BE

from bev_entry_cases import case, densify

pytestmark = pytest.mark.gpu

SPARSE_CASES = ["corners", "mixed", "empty_sample", "n0", "full", "plan", "d1", "d3"]


@pytest.fixture(scope="module", autouse=True)
def allocator_left_as_found():
    """The shared results are dropped and the caching allocator's free blocks go back to the driver when this file is done: tests of other
    files assert on peak-memory rises (tests/test_dcn_half_gpu.py), and a request served from an unsplit larger cached block counts with
    the whole block (measured: 3 538 944 bytes alone, 4 227 072 after this file without the release)."""
    yield
    sparse_run.cache_clear()
    bounds.cache_clear()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


def tensor(c, requires_grad=True):
    b, d, h, w = c["geom"]
    f = c["features"].cuda().requires_grad_(requires_grad)
    return spconv.SparseConvTensor(f, c["indices"].cuda(), [d, h, w], b), f


def run(fn, c):
    """fn(sp, weight) on fresh copies of the case's inputs -> y, dX, dW."""
    sp, f = tensor(c)
    w = c["weight"].cuda().requires_grad_(True)
    y = fn(sp, w)
    dx, dw = torch.autograd.grad(y, [f, w], c["grad"].cuda())
    return dict(y=y.detach(), dx=dx, dw=dw)


@functools.lru_cache(maxsize=None)
def bounds(name):
    c = case(name)
    t32 = run(BE.dense_route, c)
    out = {}
    for n, t in t32.items():
        e = (t.double().cpu() - c["refs"][n]).abs().max().item() if t.numel() else 0.0
        out[n] = 2 * e + 1e-6
        print(f"case {name} {n}: E(torch fp32) = {e:.3e}")
    return out


def check(name, got, keys=("y", "dx", "dw")):
    c, bd = case(name), bounds(name)
    bad = []
    for n in keys:
        ref = c["refs"][n]
        assert got[n].shape == ref.shape and (n != "y" or got[n].is_contiguous()), (n, got[n].shape, ref.shape)
        err = (got[n].double().cpu() - ref).abs().max().item() if ref.numel() else 0.0
        print(f"case {name} {n}: op error {err:.3e}, bound {bd[n]:.3e}")
        if not err <= bd[n]:
            bad.append((n, err, bd[n]))
    assert not bad, bad


@functools.lru_cache(maxsize=None)
def sparse_run(name):
    """The op on the sparse route (tau = 1) for one case: run once, shared by the per-tensor tests."""
    before = BE.ROUTES["sparse"]
    got = run(lambda sp, w: spconv.bev_entry_conv(sp, w, tau=1.0), case(name))
    assert BE.ROUTES["sparse"] == before + 1, "the sparse route declined a case it must take"
    return got


@pytest.mark.parametrize("which", ["y", "dx", "dw"])
@pytest.mark.parametrize("name", SPARSE_CASES)
def test_sparse_route_matches_float64(gpu, name, which):
    got = sparse_run(name)
    check(name, got, (which,))
    if name == "n0":
        assert not got[which].any()


def test_both_front_ends_give_the_same_bits(gpu):
    """The tables come from the compiled binding (fv2p_torch.so) or, without it, from ctypes: same kernels, same results."""
    import fv2p_native
    c = case("plan")
    ext = fv2p_native.torch_ext()
    assert ext is not None, "lib/fv2p_torch.so is missing: build with __graft_entry__.build()"
    a = sparse_run("plan")
    fv2p_native._EXT = None
    try:
        b = run(lambda sp, w: spconv.bev_entry_conv(sp, w, tau=1.0), c)
    finally:
        fv2p_native._EXT = ext
    for n in a:
        assert torch.equal(a[n], b[n]), n


@pytest.mark.parametrize("name", ["mixed", "plan"])
def test_two_calls_are_bit_identical(gpu, name):
    c = case(name)
    a = run(lambda sp, w: spconv.bev_entry_conv(sp, w, tau=1.0), c)
    b = run(lambda sp, w: spconv.bev_entry_conv(sp, w, tau=1.0), c)
    for n in a:
        assert torch.equal(a[n], b[n]), n


def test_tables_are_the_definition(gpu):
    """tab_out / tab_in / pair lists of fv2p_bev_entry_tables against their definition written with torch on the CPU."""
    c = case("mixed")
    b, d, h, w = c["geom"]
    ind = c["indices"]
    n, kvol = ind.shape[0], 9 * d
    tab_out, tab_in, pairs, num = BE._tables(ind.cuda(), c["geom"], True, False)
    want_in = torch.full((kvol, n), -1, dtype=torch.int32)
    want_out = torch.full((kvol, b * h * w), -1, dtype=torch.int32)
    for r, (ib, iz, iy, ix) in enumerate(ind.tolist()):
        for ky in range(3):
            for kx in range(3):
                oy, ox = iy + 1 - ky, ix + 1 - kx
                if 0 <= oy < h and 0 <= ox < w:
                    k, cell = iz * 9 + ky * 3 + kx, (ib * h + oy) * w + ox
                    want_in[k, r], want_out[k, cell] = cell, r
    assert torch.equal(tab_in.cpu(), want_in) and torch.equal(tab_out.cpu(), want_out)
    num = num.cpu()
    assert torch.equal(num, (want_in >= 0).sum(1).int())
    for k in range(kvol):
        rows = (want_in[k] >= 0).nonzero().squeeze(1)
        assert torch.equal(pairs[k, 0, :num[k]].cpu(), rows.int()) and torch.equal(pairs[k, 1, :num[k]].cpu(), want_in[k, rows])


def test_undispatched_shape_takes_the_dense_route(gpu):
    c = case("odd_channels")
    sp, _ = tensor(c, False)
    assert BE.route(sp, c["weight"].cuda(), tau=1.0) == "dense"
    before = BE.ROUTES["dense"]
    got = run(lambda sp, w: spconv.bev_entry_conv(sp, w, tau=1.0), c)
    assert BE.ROUTES["dense"] == before + 1
    check("odd_channels", got)


def test_fill_above_tau_takes_the_dense_route(gpu):
    c = case("dense_fill")
    sp, _ = tensor(c, False)
    assert sp.sparity > BE.TAU and BE.route(sp, c["weight"].cuda()) == "dense" and BE.route(sp, c["weight"].cuda(), tau=1.0) == "sparse"
    before = BE.ROUTES["dense"]
    got = run(spconv.bev_entry_conv, c)
    assert BE.ROUTES["dense"] == before + 1
    check("dense_fill", got)
    sparse = case("d1")
    sp, _ = tensor(sparse, False)
    assert sp.sparity <= BE.TAU and BE.route(sp, sparse["weight"].cuda()) == "sparse"


class _SmallBev(fm.FV2PConfig):
    bev_layers, bev_strides, bev_filters = (1, 1), (1, 2), (16, 32)
    bev_up_strides, bev_up_filters = (1, 2), (16, 16)


def test_bev_backbone_fed_sparse_and_dense_agree(gpu):
    """BEVBackbone on a small config: fed the sparse tensor (first conv on the sparse route) and fed dense().view(...), against the same
    network in float64 on the CPU; output and every parameter gradient of the sparse-fed run within 2 E + 1e-6, E the dense-fed run's error."""
    torch.manual_seed(5)
    b, d, h, w, c = 2, 2, 16, 12, 16
    cells = torch.randperm(b * d * h * w)[:48].sort().values
    ind = torch.stack([cells // (d * h * w), cells // (h * w) % d, cells // w % h, cells % w], 1).int()
    feats = torch.randn(ind.shape[0], c)
    net = fm.BEVBackbone(_SmallBev, c * d)
    gout = torch.randn(b, net.num_bev_features, h, w)

    def grads(m, x, g):
        m.train()
        y = m(x)
        y.backward(g)
        return [y.detach()] + [p.grad for p in m.parameters()]

    ref = grads(copy.deepcopy(net).double(), densify(feats.double(), ind, (b, d, h, w)), gout.double())
    sp = spconv.SparseConvTensor(feats.cuda(), ind.cuda(), [d, h, w], b)
    dense_fed = grads(copy.deepcopy(net).cuda(), fm.BEVBackbone.height_compression(sp), gout.cuda())
    before = BE.ROUTES["sparse"]
    sparse_fed = grads(copy.deepcopy(net).cuda(), sp, gout.cuda())
    assert BE.ROUTES["sparse"] == before + 1, "the backbone did not take the sparse route for its first conv"
    names = ["y"] + [n for n, _ in net.named_parameters()]
    bad = []
    for n, r, dn, s in zip(names, ref, dense_fed, sparse_fed):
        e = (dn.double().cpu() - r).abs().max().item()
        err = (s.double().cpu() - r).abs().max().item()
        print(f"backbone {n}: E(dense-fed fp32) = {e:.3e}, sparse-fed error {err:.3e}, bound {2 * e + 1e-6:.3e}")
        if not err <= 2 * e + 1e-6:
            bad.append((n, err, 2 * e + 1e-6))
    assert not bad, bad
