"""GPU: Linear(bias=False) -> BatchNorm1d [-> ReLU] on point rows as one op (pcdet.ops.spconv.linear, csrc/linear_bn.hip) against float64.

The truth is torch on the CPU in float64 - the same nn.Linear, nn.BatchNorm1d and nn.ReLU modules, `.double()` - and a second CPU run
in float32 is the yardstick: every compared tensor has to satisfy rel_l2(hip, f64) <= max(K * rel_l2(host32, f64), FLOOR)
(tests/f64_calibration.py).  ReLU decisions must not turn rounding into a verdict: for the gradient comparisons dy is zeroed where the
float64 pre-activation is within 1e-5 of zero (at most 1e-4 of the elements; unit-variance pre-activations give about 8e-6)."""
import copy
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn

import fv2p_native as nat
from f64_calibration import FLOOR, K, rel_l2
from pcdet.ops.spconv import linear

SPLIT_ROWS = 300    # (., 64, 128): three 128-row chunks of the weight gradient, the last one 44 rows (tests/test_linear_bn_cpu.py)
TAILS = [(2, 1, 1), (3, 5, 7), (130, 6, 20)]
WAVE = [(63, 16, 16), (64, 16, 16), (65, 17, 33)]
DECODER = [(257, 160, 192), (1031, 256, 256), (1031, 16, 128), (515, 192, 160)]
LIMITS = [(70, 1024, 512)]
SPLITS = [(SPLIT_ROWS, 64, 128)]
SHAPES = TAILS + WAVE + DECODER + LIMITS + SPLITS


def _modules(cin, cout, relu, affine=True, track=True, momentum=0.01, seed=0):
    g = torch.Generator().manual_seed(1000 + seed)
    lin = nn.Linear(cin, cout, bias=False)
    bn = nn.BatchNorm1d(cout, eps=1e-3, momentum=momentum, affine=affine, track_running_stats=track)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(cout, cin, generator=g) / cin ** 0.5)
        if affine:
            bn.weight.copy_(0.5 + torch.rand(cout, generator=g))
            bn.bias.copy_(0.3 * torch.randn(cout, generator=g))
        if track:
            bn.running_mean.copy_(0.5 * torch.randn(cout, generator=g))
            bn.running_var.copy_(0.5 + torch.rand(cout, generator=g))
    return lin, bn, (nn.ReLU() if relu else None)


def _host(mods, x, dy, dtype):
    """The three modules on the CPU in `dtype`: -> dict of outputs and gradients (+ the pre-activation and the module copies)."""
    lin, bn, relu = [None if m is None else copy.deepcopy(m).to(dtype) for m in mods]
    xx = x.detach().to(dtype).requires_grad_(True)
    pre = bn(lin(xx))
    y = relu(pre) if relu is not None else pre
    out = {"y": y.detach(), "pre": pre.detach()}
    if dy is not None:
        y.backward(dy.to(dtype))
        out.update(dx=xx.grad, dw=lin.weight.grad)
        if bn.weight is not None:
            out.update(dgamma=bn.weight.grad, dbeta=bn.bias.grad)
    if bn.running_mean is not None:
        out.update(running_mean=bn.running_mean.clone(), running_var=bn.running_var.clone(), nbt=int(bn.num_batches_tracked))
    out["mods"] = (lin, bn, relu)
    return out


def _masked_dy(pre64, relu, seed):
    """dy with zeros where the float64 pre-activation is too close to the ReLU's corner to be decided in float32."""
    g = torch.Generator().manual_seed(2000 + seed)
    dy = torch.randn(pre64.shape, generator=g)
    if relu:
        near = pre64.abs() < 1e-5
        assert int(near.sum()) <= 1e-4 * near.numel(), (int(near.sum()), near.numel())
        dy = dy.masked_fill(near, 0.0)
    return dy


def _hip(mods, x, dy, gpu, x_grad=True):
    lin, bn, relu = [None if m is None else copy.deepcopy(m).to(gpu) for m in mods]
    xx = x.detach().to(gpu).requires_grad_(x_grad)
    y = linear.linear_bn_relu(lin, bn, xx, relu)
    assert y is not None and type(y.grad_fn).__name__ == "_LinearBatchNormReLUBackward"
    saved = y.grad_fn.saved_tensors   # x, z, mean, invstd, w, gamma, beta
    out = {"y": y.detach(), "mean": saved[2].clone(), "invstd": saved[3].clone()}
    if dy is not None:
        y.backward(dy.to(gpu))
        out.update(dx=xx.grad, dw=lin.weight.grad)
        if bn.weight is not None:
            out.update(dgamma=bn.weight.grad, dbeta=bn.bias.grad)
    if bn.running_mean is not None:
        out.update(running_mean=bn.running_mean.clone(), running_var=bn.running_var.clone(), nbt=int(bn.num_batches_tracked))
    out["mods"] = (lin, bn, relu)
    return out


def _check(names, hip, h32, f64, what):
    bad = []
    for k in names:
        d_hip, d_ref = rel_l2(hip[k], f64[k]), rel_l2(h32[k], f64[k])
        print(f"{what} {k:13s} hip {d_hip:.2e}  host32 {d_ref:.2e}  bound {max(K * d_ref, FLOOR):.2e}")
        if not d_hip <= max(K * d_ref, FLOOR):
            bad.append(f"{k}: {d_hip:.2e} from float64, the host float32 run {d_ref:.2e}")
    assert not bad, (what, bad)


def _batch_stats(weight, x, eps=1e-3):
    """mean / invstd (biased variance) of the product x * weight^T, in the dtype of its arguments."""
    z = x @ weight.detach().t()
    return z.mean(0), 1.0 / torch.sqrt(z.var(0, unbiased=False) + eps)


def _case(gpu, n, cin, cout, relu, affine=True, track=True, momentum=0.01, seed=0):
    mods = _modules(cin, cout, relu, affine, track, momentum, seed)
    x = torch.randn(n, cin, generator=torch.Generator().manual_seed(3000 + seed))
    pre64 = _host(mods, x, None, torch.float64)["pre"]
    dy = _masked_dy(pre64, relu, seed)
    f64, h32 = _host(mods, x, dy, torch.float64), _host(mods, x, dy, torch.float32)
    hip = _hip(mods, x, dy, gpu)
    f64["mean"], f64["invstd"] = _batch_stats(f64["mods"][0].weight, x.double())
    h32["mean"], h32["invstd"] = _batch_stats(h32["mods"][0].weight, x)
    names = ["y", "dx", "dw", "mean", "invstd"] + (["dgamma", "dbeta"] if affine else []) + (["running_mean", "running_var"] if track else [])
    _check(names, hip, h32, f64, f"({n}, {cin}, {cout}) relu={relu} affine={affine} track={track} momentum={momentum}")
    if track:
        assert hip["nbt"] == f64["nbt"] == 1
    return hip, h32, f64


@pytest.mark.gpu
@pytest.mark.parametrize("n,cin,cout", SHAPES)
def test_training_mode_against_float64(gpu, n, cin, cout):
    """Every shape class: tails on all three extents, around one wave / workgroup tile, the decoder's channel pairs with ragged rows,
    the limits, and three weight-gradient chunks with a ragged last one; with ReLU + affine + tracked statistics, and without any."""
    if (n, cin, cout) in SPLITS:
        s = nat.call("fv2p_linear_bn_splits", n, cin, cout)
        assert s >= 3 and n % 128 != 0
    _case(gpu, n, cin, cout, relu=True)
    _case(gpu, n, cin, cout, relu=False, affine=False, track=False, seed=1)


@pytest.mark.gpu
@pytest.mark.parametrize("relu,affine,track", [(False, True, True), (True, False, True), (True, True, False)])
def test_module_options(gpu, relu, affine, track):
    for n, cin, cout in [(130, 6, 20), (65, 17, 33), (257, 160, 192)]:
        _case(gpu, n, cin, cout, relu=relu, affine=affine, track=track, seed=2)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3, 65])
@pytest.mark.parametrize("momentum", [0.01, 1.0, None])
def test_running_statistics(gpu, n, momentum):
    """torch's update: the unbiased variance (factor 1.5 at n = 3, which momentum 1.0 shows undiluted), the cumulative average for
    momentum=None (two calls), num_batches_tracked + 1 per training call and none in eval mode."""
    cin, cout = 5, 7
    mods = _modules(cin, cout, True, momentum=momentum, seed=4)
    ref64 = [copy.deepcopy(m).double() for m in mods]
    ref32 = [copy.deepcopy(m) for m in mods]
    dev = [copy.deepcopy(m).to(gpu) for m in mods]
    for call in range(2):
        x = torch.randn(n, cin, generator=torch.Generator().manual_seed(4000 + call))
        ref64[2](ref64[1](ref64[0](x.double())))
        ref32[2](ref32[1](ref32[0](x)))
        assert linear.linear_bn_relu(dev[0], dev[1], x.to(gpu), dev[2]) is not None
        assert int(dev[1].num_batches_tracked) == call + 1 == int(ref64[1].num_batches_tracked)
        hip = {"running_mean": dev[1].running_mean, "running_var": dev[1].running_var}
        h32 = {"running_mean": ref32[1].running_mean, "running_var": ref32[1].running_var}
        f64 = {"running_mean": ref64[1].running_mean, "running_var": ref64[1].running_var}
        _check(["running_mean", "running_var"], hip, h32, f64, f"n={n} momentum={momentum} call {call}")
    for m in dev:
        m.eval()
    before = (dev[1].running_mean.clone(), dev[1].running_var.clone())
    assert linear.linear_bn_relu(dev[0], dev[1], torch.randn(n, cin, device=gpu), dev[2]) is not None
    assert int(dev[1].num_batches_tracked) == 2
    assert torch.equal(dev[1].running_mean, before[0]) and torch.equal(dev[1].running_var, before[1])


@pytest.mark.gpu
def test_large_mean(gpu):
    """|mean| about 300 standard deviations per channel: sums of squares kept in fp32 lose the variance."""
    n, cin, cout = 257, 16, 20
    mods = _modules(cin, cout, False, seed=5)
    g = torch.Generator().manual_seed(5000)
    with torch.no_grad():
        mods[0].weight.copy_((1.0 + 0.1 * torch.randn(cout, cin, generator=g)) / cin ** 0.5)
    x = torch.randn(n, cin, generator=g) + 300.0 / cin ** 0.5
    z = x.double() @ mods[0].weight.detach().double().t()
    ratio = z.mean(0).abs() / z.std(0)
    assert 200.0 < float(ratio.min()) and float(ratio.max()) < 400.0, ratio
    f64, h32 = _host(mods, x, None, torch.float64), _host(mods, x, None, torch.float32)
    hip = _hip(mods, x, None, gpu)
    f64["invstd"] = 1.0 / torch.sqrt(z.var(0, unbiased=False) + 1e-3)
    z32 = x @ mods[0].weight.detach().t()
    h32["invstd"] = 1.0 / torch.sqrt(z32.var(0, unbiased=False) + 1e-3)
    _check(["y", "invstd"], hip, h32, f64, "large mean")


@pytest.mark.gpu
@pytest.mark.parametrize("n,cin,cout", [(1, 5, 7), (65, 17, 33), (515, 192, 160)])
def test_eval_mode(gpu, n, cin, cout):
    """Forward in one launch from the running statistics, and the backward pass through the frozen BatchNorm (batch_stats = 0)."""
    mods = [m.eval() for m in _modules(cin, cout, True, seed=6)]
    x = torch.randn(n, cin, generator=torch.Generator().manual_seed(6000))
    pre64 = _host(mods, x, None, torch.float64)["pre"]
    dy = _masked_dy(pre64, True, 6)
    f64, h32 = _host(mods, x, dy, torch.float64), _host(mods, x, dy, torch.float32)
    hip = _hip(mods, x, dy, gpu)
    _check(["y", "dx", "dw", "dgamma", "dbeta"], hip, h32, f64, f"eval ({n}, {cin}, {cout})")
    assert hip["nbt"] == 0
    assert torch.equal(hip["running_mean"].cpu(), mods[1].running_mean) and torch.equal(hip["running_var"].cpu(), mods[1].running_var)


@pytest.mark.gpu
def test_eval_mode_without_grad_keeps_no_pre_activation(gpu):
    n, cin, cout = 64, 16, 16    # one n x cout tensor is 4096 bytes: a whole number of the allocator's blocks
    lin, bn, relu = [m.eval().to(gpu) for m in _modules(cin, cout, True, seed=7)]
    x = torch.randn(n, cin, device=gpu)
    with torch.no_grad():
        linear.linear_bn_relu(lin, bn, x, relu)   # (the library is loaded, the allocator warm)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        y = linear.linear_bn_relu(lin, bn, x, relu)
        after = torch.cuda.memory_allocated()
    assert y is not None and after - before == n * cout * 4, (before, after)
    before = torch.cuda.memory_allocated()
    y2 = linear.linear_bn_relu(lin, bn, x, relu)    # a gradient can be asked for: y, z and the two [cout] vectors stay
    after = torch.cuda.memory_allocated()
    assert after - before >= 2 * n * cout * 4 and torch.equal(y, y2)


def _grads(gpu, mods, x, dy, x_grad=True, w_grad=True):
    lin, bn, relu = [None if m is None else copy.deepcopy(m).to(gpu) for m in mods]
    lin.weight.requires_grad_(w_grad)
    xx = x.to(gpu).requires_grad_(x_grad)
    y = linear.linear_bn_relu(lin, bn, xx, relu)
    y.backward(dy.to(gpu))
    return {"y": y.detach(), "dx": xx.grad, "dw": lin.weight.grad, "dgamma": bn.weight.grad, "dbeta": bn.bias.grad,
            "running_mean": bn.running_mean, "running_var": bn.running_var}


@pytest.mark.gpu
def test_needs_input_grad(gpu):
    n, cin, cout = 130, 6, 20
    mods = _modules(cin, cout, True, seed=8)
    x, dy = torch.randn(n, cin), torch.randn(n, cout)
    full = _grads(gpu, mods, x, dy)
    no_x = _grads(gpu, mods, x, dy, x_grad=False)
    no_w = _grads(gpu, mods, x, dy, w_grad=False)
    assert no_x["dx"] is None and no_w["dw"] is None and full["dx"] is not None and full["dw"] is not None
    for k in ("y", "dw", "dgamma", "dbeta"):
        assert torch.equal(no_x[k], full[k]), k
    for k in ("y", "dx", "dgamma", "dbeta"):
        assert torch.equal(no_w[k], full[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("n,cin,cout", [(1031, 256, 256), (SPLIT_ROWS, 64, 128), (65, 17, 33)])
def test_run_to_run_bits(gpu, n, cin, cout):
    """Forward + backward twice from identical copies of the modules, no library determinism settings: the same bits."""
    mods = _modules(cin, cout, True, seed=9)
    x, dy = torch.randn(n, cin), torch.randn(n, cout)
    a = _grads(gpu, mods, x, dy)
    junk = torch.randn(1 << 20, device=gpu)   # other contents in the allocator's blocks between the two runs
    b = _grads(gpu, mods, x, dy)
    del junk
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


@pytest.mark.gpu
def test_declines(gpu):
    """Every situation that is not the plain one: None, and the modules' buffers untouched."""
    cin, cout, n = 6, 10, 9
    x = torch.randn(n, cin, device=gpu)

    def mk(**kw):
        lin, bn, relu = _modules(cin, cout, True, **kw)
        return [lin.to(gpu), bn.to(gpu), relu]

    def declined(lin, bn, relu, xin):
        before = {k: v.clone() for k, v in bn.state_dict().items()}
        assert linear.fusable(lin, bn, relu, xin) is False
        assert linear.linear_bn_relu(lin, bn, xin, relu) is None
        for k, v in bn.state_dict().items():
            assert torch.equal(v, before[k]), k

    lin, bn, relu = mk()
    assert linear.fusable(lin, bn, relu, x) is True
    declined(nn.Linear(cin, cout, bias=True).to(gpu), bn, relu, x)                   # a Linear with bias

    class MyLinear(nn.Linear):
        pass
    declined(MyLinear(cin, cout, bias=False).to(gpu), bn, relu, x)                   # a Linear subclass
    for which in range(3):                                                           # a hook on any of the three
        mods = mk()
        mods[which].register_forward_hook(lambda m, i, o: None)
        declined(*mods, x)
    for which in range(3):                                                           # forward replaced on the instance
        mods = mk()
        mods[which].forward = lambda t: t
        declined(*mods, x)
    declined(lin, bn, relu, torch.randn(cin, n, device=gpu).t())                     # non-contiguous rows
    declined(lin, bn, relu, x.half())                                                # float16 rows
    with torch.autocast("cuda", dtype=torch.float16):
        declined(lin, bn, relu, x)
    declined(lin, bn, relu, x[:1])                                                   # one row in training mode: torch's error stays torch's
    ev = [m.eval() for m in mk()]
    assert linear.linear_bn_relu(ev[0], ev[1], x[:1].contiguous(), ev[2]) is not None   # ... the same rows in eval mode run
    declined(lin, nn.BatchNorm1d(cout + 1).to(gpu), relu, x)                         # mismatched num_features
    declined(lin, nn.BatchNorm1d(cout).to(gpu).double(), relu, x)                    # parameters of another dtype
    declined(nn.Linear(cin, cout, bias=False).to(gpu).half(), bn, relu, x)
    saved = linear._ENABLED
    try:
        linear._ENABLED = False
        declined(lin, bn, relu, x)
    finally:
        linear._ENABLED = saved


@pytest.mark.gpu
def test_limits(gpu):
    """cin 1025 and cout 513: None from Python, FV2P_EINVAL from the C entry points (the shape is judged before any pointer)."""
    x = torch.randn(4, 1025, device=gpu)
    assert linear.linear_bn_relu(nn.Linear(1025, 8, bias=False).to(gpu), nn.BatchNorm1d(8).to(gpu), x) is None
    x = torch.randn(4, 8, device=gpu)
    assert linear.linear_bn_relu(nn.Linear(8, 513, bias=False).to(gpu), nn.BatchNorm1d(513).to(gpu), x) is None
    lib = nat.lib()
    for n, cin, cout in [(4, 1025, 8), (4, 8, 513), (4, 0, 8), (0, 8, 8)]:
        assert lib.fv2p_linear_bn_forward(None, n, cin, None, cout, 1e-3, 0.01, None, None, 1, None, None, None, None, None, None, None, None, 0, None) == -1
        assert "fv2p_linear_bn_forward" in nat.last_error()
        assert lib.fv2p_linear_bn_forward_eval(None, n, cin, None, cout, None, None, None, None, 1, None, None, None) == -1
        assert lib.fv2p_linear_bn_backward(None, None, None, n, cin, None, cout, None, None, None, None, 1, 1, None, None, None, None, None, None, 0, None) == -1
    assert lib.fv2p_linear_bn_forward(None, 1, 8, None, 8, 1e-3, 0.01, None, None, 1, None, None, None, None, None, None, None, None, 0, None) == -1   # n = 1


def _count_nodes(fn, name):
    seen, stack, count = set(), [fn], 0
    while stack:
        f = stack.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        count += type(f).__name__ == name
        stack.extend(g for g, _ in f.next_functions)
    return count


def _seq_grads(seq, x, dy, dtype, device, run):
    seq = copy.deepcopy(seq).to(device=device, dtype=dtype)
    out = run(seq, x.to(device=device, dtype=dtype))
    out.backward(dy.to(device=device, dtype=dtype))
    res = {"out": out.detach()}
    res.update({k: p.grad for k, p in seq.named_parameters()})
    return res, out


@pytest.mark.gpu
def test_run_rows_on_a_lateral_block(gpu, monkeypatch):
    from fv2p_harness import fv2p_model
    torch.manual_seed(10)
    seq = nn.Sequential(nn.Linear(64, 192, bias=False), nn.BatchNorm1d(192, eps=1e-3, momentum=0.01), nn.ReLU(),
                        nn.Linear(192, 192, bias=False), nn.BatchNorm1d(192, eps=1e-3, momentum=0.01))
    x = torch.randn(515, 64)
    dy = torch.randn(515, 192)
    plain = lambda s, t: s(t)
    f64, _ = _seq_grads(seq, x, dy, torch.float64, "cpu", plain)
    h32, _ = _seq_grads(seq, x, dy, torch.float32, "cpu", plain)
    monkeypatch.setattr(linear, "pays", lambda n, cin, cout: True)
    for run in (linear.run_rows, fv2p_model.run_rows):
        hip, out = _seq_grads(seq, x, dy, torch.float32, gpu, run)
        assert _count_nodes(out.grad_fn, "_LinearBatchNormReLUBackward") == 2
        _check(list(f64), hip, h32, f64, run.__module__ + ".run_rows")
    monkeypatch.setattr(linear, "pays", lambda n, cin, cout: False)
    _, out = _seq_grads(seq, x, dy, torch.float32, gpu, linear.run_rows)
    assert _count_nodes(out.grad_fn, "_LinearBatchNormReLUBackward") == 0


@pytest.mark.gpu
def test_bev_grid_pooling_compression(gpu, monkeypatch):
    from pcdet.models.backbones_3d.pfe import bev_grid_pooling as bgp
    torch.manual_seed(11)
    mod = bgp.BEVGridPooling(SimpleNamespace(IN_CHANNELS=16, OUT_CHANNELS=8), [0.0, -40.0, -3.0, 70.4, 40.0, 1.0], [0.05, 0.05, 0.1])
    bev = torch.randn(2, 16, 25, 22, device=gpu)
    kp = torch.rand(2, 300, 3, device=gpu) * torch.tensor([8.0, 8.0, 1.0], device=gpu) + torch.tensor([0.0, -40.0, -2.0], device=gpu)
    dy = torch.randn(2, 300, 8)
    seq = mod.point_bev_feature_compress
    feats = mod.interpolate_from_bev_features(kp, bev, 2, 8).reshape(600, 16).cpu()
    plain = lambda s, t: s(t)
    f64, _ = _seq_grads(seq, feats, dy.view(600, 8), torch.float64, "cpu", plain)
    h32, _ = _seq_grads(seq, feats, dy.view(600, 8), torch.float32, "cpu", plain)
    monkeypatch.setattr(linear, "pays", lambda n, cin, cout: True)
    dev = copy.deepcopy(mod).to(gpu)
    out = dev({"spatial_features_before_head": bev, "spatial_features_stride": 8, "batch_size": 2}, kp)
    assert out.shape == (2, 300, 8) and _count_nodes(out.grad_fn, "_LinearBatchNormReLUBackward") == 1
    out.backward(dy.to(gpu))
    hip = {"out": out.detach().view(600, 8)}
    hip.update({k: p.grad for k, p in dev.point_bev_feature_compress.named_parameters()})
    _check(list(f64), hip, h32, f64, "BEVGridPooling")
