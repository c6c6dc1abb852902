"""Deterministic mode (pcdet.ops.set_deterministic) on the GPU.

fv2p_scatter_add against a host restatement of its documented order, bit for bit; every backward that otherwise adds with float
atomics, in its fixed-order form: (a) against a float64 restatement within 1e-4 of the largest entry, (b) bit-identical over five calls
on "hub" inputs (tens of thousands of contributions on a handful of rows, where atomics reorder), (c) bit-identical when the call runs on
a second stream while the first one is busy, (d) edge shapes.  Last, the reduced FV2P and MGAF training steps twice in one process with
the mode on: loss and every parameter gradient bit-identical."""
import contextlib

import numpy as np
import pytest
import torch

import fv2p_native as _nat
import pcdet.ops as ops

pytestmark = pytest.mark.gpu
TOL = 1e-4
REPEATS = 5


@contextlib.contextmanager
def mode(on):
    was = ops.is_deterministic()
    ops.set_deterministic(on)
    try:
        yield
    finally:
        ops.set_deterministic(was)


def rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want).max() / max(np.abs(want).max(), 1e-12)


def repeat_and_side_stream(fn):
    """fn() -> tuple of tensors.  Five calls on the current stream, then one on a second stream while the first one runs a queue of
    matrix products; every result must equal the first, bit for bit.  Returns the first result (host copies)."""
    first = [t.detach().cpu() for t in fn()]
    for _ in range(REPEATS - 1):
        again = [t.detach().cpu() for t in fn()]
        for a, b in zip(first, again):
            assert torch.equal(a, b), "fixed-order form differs between two identical calls"
    dev = torch.device("cuda", torch.cuda.current_device())
    big = torch.randn(2048, 2048, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for _ in range(8):
        big = (big @ big).tanh_()
    with torch.cuda.stream(side):
        res = fn()
    side.synchronize()
    torch.cuda.synchronize()
    for a, b in zip(first, res):
        assert torch.equal(a, b.detach().cpu()), "fixed-order form differs on a second stream"
    return first


# ---- the primitive -----------------------------------------------------------------------------------------------------------------
def host_scatter(dst, off, coef, src, cs, c, n_dst, out):
    """The documented order, restated: kept entries sorted by (row, entry), cut into 32-position segments; a row's piece of a segment
    summed from zero as acc = acc + coef * value (float32, two roundings); pieces added in segment order; out = out + total."""
    out = out.astype(np.float32).copy().reshape(n_dst, c)
    e = np.nonzero((dst >= 0) & (dst < n_dst))[0]
    e = e[np.lexsort((e, dst[e]))]
    rows = dst[e]
    chans = np.arange(c) * cs
    p = 0
    while p < len(e):
        q = p
        while q < len(e) and rows[q] == rows[p]:
            q += 1
        pieces = []
        for seg in range(p // 32, (q - 1) // 32 + 1):
            acc = np.zeros(c, np.float32)
            for i in range(max(p, seg * 32), min(q, seg * 32 + 32)):
                w = np.float32(1.0) if coef is None else coef[e[i]]
                o = e[i] * c if off is None else off[e[i]]
                acc = acc + w * src[o + chans]
            pieces.append(acc)
        total = pieces[0]
        for piece in pieces[1:]:
            total = total + piece
        out[rows[p]] = out[rows[p]] + total
        p = q
    return out


def scatter(dst, off, coef, src, cs, c, n_dst, out):
    entries = dst.numel()
    ws = _nat.workspace(_nat.lib().fv2p_scatter_add_ws_bytes(entries, c), dst.device)
    _nat.call("fv2p_scatter_add", entries, c, n_dst, dst, off, coef, src, cs, out, ws, ws.numel(), _nat.stream())
    return out


@pytest.mark.parametrize("entries,c,n_dst,hub", [(5000, 16, 7, True), (3000, 3, 500, False), (70, 64, 2, True), (1, 5, 4, False),
                                                 (0, 8, 4, False), (4000, 1, 3, True)])
@pytest.mark.parametrize("unaligned", [False, True])
def test_scatter_add_is_the_documented_order_bit_for_bit(gpu, entries, c, n_dst, hub, unaligned):
    rng = np.random.default_rng(entries + c)
    dst = rng.integers(-2, n_dst + 2, entries).astype(np.int32)   # some rows out of range: dropped
    if hub:
        dst[rng.random(entries) < 0.9] = rng.integers(0, min(3, n_dst))
    n_src = max(entries, 1) + 3
    src = rng.standard_normal(n_src * c + 1).astype(np.float32)
    off = rng.integers(0, n_src, entries).astype(np.int64) * c
    coef = rng.standard_normal(entries).astype(np.float32)
    out0 = rng.standard_normal(n_dst * c + 1).astype(np.float32)
    lead = 1 if unaligned else 0   # views one float into their storage: 16-byte accesses are off, the scalar path runs
    s_t = torch.from_numpy(src).to(gpu)[lead:lead + n_src * c]
    o_t = torch.from_numpy(out0).to(gpu)[lead:lead + n_dst * c]
    want = host_scatter(dst, off, coef, src[lead:], 1, c, n_dst, out0[lead:lead + n_dst * c])
    got = scatter(torch.from_numpy(dst).to(gpu), torch.from_numpy(off).to(gpu), torch.from_numpy(coef).to(gpu), s_t, 1, c, n_dst,
                  o_t.clone()).cpu().numpy().reshape(n_dst, c)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # no offsets and no coefficients: src is [entries, c], every coefficient 1
    want = host_scatter(dst, None, None, src[lead:], 1, c, n_dst, out0[lead:lead + n_dst * c])
    got = scatter(torch.from_numpy(dst).to(gpu), None, None, s_t, 1, c, n_dst, o_t.clone()).cpu().numpy().reshape(n_dst, c)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_scatter_add_channel_stride(gpu):
    """src_cs > 1: a channel-major source, the layout of the batch pointnet2 gradients."""
    rng = np.random.default_rng(3)
    entries, c, n_dst, cols = 900, 6, 5, 900
    src = rng.standard_normal(c * cols).astype(np.float32)   # [c][cols]
    dst = rng.integers(0, n_dst, entries).astype(np.int32)
    off = np.arange(entries, dtype=np.int64)
    want = host_scatter(dst, off, None, src, cols, c, n_dst, np.zeros(n_dst * c, np.float32))
    got = scatter(torch.from_numpy(dst).to(gpu), torch.from_numpy(off).to(gpu), None, torch.from_numpy(src).to(gpu), cols, c, n_dst,
                  torch.zeros(n_dst * c, device=gpu)).cpu().numpy().reshape(n_dst, c)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- per op --------------------------------------------------------------------------------------------------------------------------
def backward_of(op, inputs, grad, which):
    """Gradients of `op(*inputs)` for the inputs at positions `which`, with the mode on."""
    def run():
        xs = [t.detach().clone().requires_grad_(i in which) if torch.is_tensor(t) and t.is_floating_point() else t
              for i, t in enumerate(inputs)]
        with mode(True):
            out = op(*xs)
            out = out[0] if isinstance(out, tuple) else out
            gs = torch.autograd.grad(out, [xs[i] for i in which], grad)
        return gs
    return run


def test_group_points_stack(gpu):
    from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils as st
    rng = np.random.default_rng(0)
    n, m, s, c = 40, 3000, 16, 13                      # 48 000 contributions: 90 % on three points
    feats = torch.randn(n, c, device=gpu)
    fcnt = torch.tensor([25, 15], dtype=torch.int32, device=gpu)
    icnt = torch.tensor([2000, 1000], dtype=torch.int32, device=gpu)
    idx = rng.integers(0, 15, (m, s)).astype(np.int32)
    idx[rng.random((m, s)) < 0.9] = rng.integers(0, 3)
    idx_t = torch.from_numpy(idx).to(gpu)
    grad = torch.randn(m, c, s, device=gpu)
    (got,) = repeat_and_side_stream(backward_of(lambda f: st.GroupingOperation.apply(f, fcnt, idx_t, icnt), [feats], grad, [0]))
    start = np.where(np.arange(m) < 2000, 0, 25)
    want = np.zeros((n, c))
    np.add.at(want, (start[:, None] + idx).reshape(-1), grad.cpu().double().numpy().transpose(0, 2, 1).reshape(-1, c))
    assert rel(got, want) < TOL


@pytest.mark.parametrize("kind", ["group", "gather", "interp"])
def test_batch_pointnet2(gpu, kind):
    from pcdet.ops.pointnet2.pointnet2_batch import pointnet2_utils as pb
    rng = np.random.default_rng(1)
    b, c, n = 2, 7, 50
    feats = torch.randn(b, c, n, device=gpu)
    if kind == "group":
        m, s = 600, 32
        idx = rng.integers(0, n, (b, m, s)).astype(np.int32)
        idx[rng.random((b, m, s)) < 0.9] = 2
        op, grad = (lambda f: pb.GroupingOperation.apply(f, torch.from_numpy(idx).to(gpu))), torch.randn(b, c, m, s, device=gpu)
        g = grad.cpu().double().numpy().reshape(b, c, -1)
        flat, w = idx.reshape(b, -1), None
    elif kind == "gather":
        m = 20000
        idx = rng.integers(0, n, (b, m)).astype(np.int32)
        idx[rng.random((b, m)) < 0.9] = 1
        op, grad = (lambda f: pb.GatherOperation.apply(f, torch.from_numpy(idx).to(gpu))), torch.randn(b, c, m, device=gpu)
        g, flat, w = grad.cpu().double().numpy(), idx, None
    else:
        q = 8000
        idx = rng.integers(0, n, (b, q, 3)).astype(np.int32)
        idx[rng.random((b, q, 3)) < 0.9] = 0
        wt = torch.rand(b, q, 3, device=gpu)
        op, grad = (lambda f: pb.ThreeInterpolate.apply(f, torch.from_numpy(idx).to(gpu), wt)), torch.randn(b, c, q, device=gpu)
        g = np.repeat(grad.cpu().double().numpy(), 3, axis=2)
        flat, w = idx.reshape(b, -1), wt.cpu().double().numpy().reshape(b, -1)
    (got,) = repeat_and_side_stream(backward_of(op, [feats], grad, [0]))
    want = np.zeros((b, c, n))
    for bb in range(b):
        for ch in range(c):
            np.add.at(want[bb, ch], flat[bb], g[bb, ch] * (1.0 if w is None else w[bb]))
    assert rel(got, want) < TOL


@pytest.mark.parametrize("channels_first", [True, False])
def test_bev_interp(gpu, channels_first):
    from pcdet.models.backbones_3d.pfe.bev_grid_pooling import _BevInterp
    b, c, h, w, n = 2, 9, 12, 10, 20000
    rng = np.random.default_rng(2)
    x = (3.0 + 0.9 * rng.random((b, n))).astype(np.float32)   # every sample inside one cell: four hub rows per sample
    y = (5.0 + 0.9 * rng.random((b, n))).astype(np.float32)
    bev = torch.randn((b, c, h, w) if channels_first else (b, h, w, c), device=gpu)
    xt, yt = torch.from_numpy(x).to(gpu), torch.from_numpy(y).to(gpu)
    grad = torch.randn(b, n, c, device=gpu)
    (got,) = repeat_and_side_stream(backward_of(lambda m: _BevInterp.apply(m, xt, yt, channels_first), [bev], grad, [0]))
    want = np.zeros((b, h, w, c))
    gd = grad.cpu().double().numpy()
    for bb in range(b):
        xx, yy = x[bb].astype(np.float64), y[bb].astype(np.float64)
        x0, y0 = np.clip(np.floor(xx).astype(int), 0, w - 1), np.clip(np.floor(yy).astype(int), 0, h - 1)
        x1, y1 = np.clip(np.floor(xx).astype(int) + 1, 0, w - 1), np.clip(np.floor(yy).astype(int) + 1, 0, h - 1)
        for (cy, cx, wt) in ((y0, x0, (x1 - xx) * (y1 - yy)), (y1, x0, (x1 - xx) * (yy - y0)), (y0, x1, (xx - x0) * (y1 - yy)),
                             (y1, x1, (xx - x0) * (yy - y0))):
            np.add.at(want[bb], (cy, cx), gd[bb] * wt[:, None])
    if channels_first:
        want = want.transpose(0, 3, 1, 2)
    assert rel(got, want) < TOL


@pytest.mark.parametrize("pool_method", [0, 1])
def test_roiaware_pool3d(gpu, pool_method):
    """Calls the entry points directly with member lists that share a handful of points (what overlapping RoIs produce)."""
    rng = np.random.default_rng(4 + pool_method)
    r, o, c, cap, p = 24, 6, 19, 33, 40
    members = np.zeros((r, o, o, o, cap), np.int32)
    cnt = rng.integers(0, cap, (r, o, o, o))
    members[..., 0] = cnt
    members[..., 1:] = np.where(rng.random((r, o, o, o, cap - 1)) < 0.9, rng.integers(0, 3, (r, o, o, o, cap - 1)),
                                rng.integers(0, p, (r, o, o, o, cap - 1)))
    argmax = np.where(rng.random((r, o, o, o, c)) < 0.1, -1, rng.integers(0, 3, (r, o, o, o, c))).astype(np.int32)
    grad = torch.randn(r, o, o, o, c, device=gpu)
    mt, at = torch.from_numpy(members).to(gpu), torch.from_numpy(argmax).to(gpu)

    def run():
        g = torch.full((p, c), float("nan"), device=gpu)   # written, not accumulated
        ws = _nat.workspace(_nat.lib().fv2p_roiaware_pool3d_bwd_ws_bytes(r, o, o, o, c, cap, pool_method), gpu)
        _nat.call("fv2p_roiaware_pool3d_bwd_gather", mt, at, grad, r, o, o, o, c, cap, pool_method, p, g, ws, ws.numel(), _nat.stream())
        return (g,)
    (got,) = repeat_and_side_stream(run)
    want = np.zeros((p, c))
    gd = grad.cpu().double().numpy().reshape(-1, c)
    mem, am = members.reshape(-1, cap), argmax.reshape(-1, c)
    for v in range(mem.shape[0]):
        if pool_method == 0:
            ok = am[v] >= 0
            np.add.at(want, (am[v][ok], np.arange(c)[ok]), gd[v][ok])
        else:
            k = mem[v, 0]
            for j in range(1, k + 1):
                want[mem[v, j]] += gd[v] / max(k, 1)
    assert rel(got, want) < TOL


@pytest.mark.parametrize("no_trans", [False, True])
def test_deform_psroi_pool(gpu, no_trans):
    from oracle import psroi_oracle as ps
    from pcdet.ops.DeformableConvolutionV2PyTorch import DCN
    rng = np.random.default_rng(6)
    bsz, c, h, w, nr = 2, 8, 20, 24, 300
    data = torch.randn(bsz, c, h, w, device=gpu)
    rois = np.zeros((nr, 5), np.float32)                 # 300 RoIs over one small patch: the same map cells over and over
    rois[:, 0] = rng.integers(0, bsz, nr)
    rois[:, 1:3] = rng.uniform(3, 5, (nr, 2))
    rois[:, 3:5] = rois[:, 1:3] + rng.uniform(3, 5, (nr, 2))
    trans = torch.from_numpy(rng.uniform(-0.1, 0.1, (nr, 2, 3, 3)).astype(np.float32)).to(gpu)
    conf = (no_trans, 1.0, c, 1, 3, 3, 4, 0.1)
    bt = torch.from_numpy(rois).to(gpu)
    out, top = DCN.deform_psroi_pooling_forward(data, bt, trans, *conf)
    grad = torch.randn_like(out)

    def run():
        with mode(True):
            return DCN.deform_psroi_pooling_backward(grad, data, bt, trans, top, *conf)
    gd, gt = repeat_and_side_stream(run)
    wd, wt = ps.deform_psroi_pooling_backward(grad.cpu().double().numpy(), data.cpu().double().numpy(), rois.astype(np.float64),
                                             trans.cpu().double().numpy(), top.cpu().double().numpy(), *conf)
    assert rel(gd, wd) < TOL
    if not no_trans:
        assert rel(gt, wt) < TOL


def test_sa_grid(gpu):
    from pcdet.ops.pointnet2.pointnet2_batch import fused
    rng = np.random.default_rng(7)
    r, n, m, s, c = 4, 300, 216, 32, 64                  # 27 648 samples: 90 % on three points of each RoI
    pp, pc = torch.randn(r, n, c, device=gpu), torch.randn(r, m, c, device=gpu)
    w2 = torch.randn(c, c, device=gpu) / 8
    idx = rng.integers(0, n, (r, m, s)).astype(np.int32)
    idx[rng.random((r, m, s)) < 0.9] = rng.integers(0, 3)
    it = torch.from_numpy(idx).to(gpu)
    grad = torch.randn(r, m, c, device=gpu)
    got = repeat_and_side_stream(backward_of(lambda a, b_, w: fused.sa_grid_max(a, b_, it, w), [pp, pc, w2], grad, [0, 1, 2]))
    P, Q, W = (t.cpu().double().requires_grad_(True) for t in (pp, pc, w2))
    g = P[torch.arange(r)[:, None, None], torch.from_numpy(idx).long()]            # [r, m, s, c]
    h = torch.relu(torch.relu(g - Q[:, :, None, :]) @ W.t()).max(2).values
    want = torch.autograd.grad(h, (P, Q, W), grad.cpu().double())
    for a, b_ in zip(got, want):
        assert rel(a, b_.numpy()) < TOL


# ---- the step ----------------------------------------------------------------------------------------------------------------------
def step_twice(build, run):
    """Two fresh models from the same seed, the same inputs, deterministic libraries and mode: (loss, gradients) per run."""
    from conftest import deterministic_libraries
    res = []
    for _ in range(2):
        torch.manual_seed(0)
        net = build()
        net.taps = {}
        with deterministic_libraries(), mode(True):
            loss = run(net)
            loss.backward()
        torch.cuda.synchronize()
        res.append((loss.detach().cpu(), {k: p.grad.detach().cpu() for k, p in net.named_parameters() if p.grad is not None}))
    (l0, g0), (l1, g1) = res
    assert torch.equal(l0, l1), (float(l0), float(l1))
    assert g0.keys() == g1.keys() and len(g0) > 50
    differ = [k for k in g0 if not torch.equal(g0[k], g1[k])]
    assert not differ, f"{len(differ)} parameter gradients differ between two runs: {differ[:8]}"


def test_fv2p_step_is_bit_identical(gpu):
    from test_fv2p_step_gpu import SmallFV2P, make_inputs
    from fv2p_harness.fv2p_model import FV2PDetector
    clouds, feats, coords, gt, u = make_inputs(SmallFV2P, 2, 4096)
    step_twice(lambda: FV2PDetector(SmallFV2P).to(gpu),
               lambda net: net([c.to(gpu) for c in clouds], feats.to(gpu), coords.to(gpu), gt.to(gpu), u.to(gpu)))


def test_mgaf_step_is_bit_identical(gpu):
    from test_mgaf_head import SmallMGAF, small_inputs
    from fv2p_harness import mgaf_model as mm
    feats, coords, gt = small_inputs()
    def build():
        net = mm.MGAFDetector(SmallMGAF).to(gpu)
        net.iou_peaks = None   # each run's own top-24 peaks (identical when the runs are)
        return net
    step_twice(build, lambda net: net(feats.to(gpu), coords.to(gpu), 2, gt.to(gpu)))
