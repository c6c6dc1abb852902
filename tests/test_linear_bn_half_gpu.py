"""GPU: Linear(bias=False) -> BatchNorm1d [-> ReLU] on float16 / bfloat16 point rows as one op (pcdet.ops.spconv.linear: fusable16,
linear_bn_relu16, _LinearBatchNormReLU16; the 16-bit formats of csrc/linear_bn.hip) against the float64 references and the derived bounds of
linear_bn_half_cases.py - nothing in a bound is measured:

  stage A  the op's stored 16-bit pre-activation z (read from the saved tensors) against x64 w64^T;
  stage B  mean, invstd, y, the running statistics, dgamma and dbeta against oracle/bn_oracle.py ON THAT z;
  stage C  dx and dw against the float64 products of the oracle's du64, the staging error of du propagated through |w| and |x|.

For the gradient comparisons dy is zeroed where the float64 pre-activation (of the op's z) is within 4 (e + 2^-24) of the ReLU's kink;
at most 1e-4 of the elements may be.  Every comparison prints its largest |err| / bound before it asserts."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

import fv2p_native as nat
import linear_bn_half_cases as cases
import pcdet.ops.spconv as spconv
from f64_calibration import FLOOR, K, rel_l2
from oracle import bn_oracle
from pcdet.ops.spconv import linear

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]
DT_CODE = {torch.float16: 1, torch.bfloat16: 2}
UNIT = cases.UNIT
NODE = "_LinearBatchNormReLU16Backward"
dtype_id = lambda d: str(d).replace("torch.", "")


def _dev(a, dtype, gpu):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(gpu).to(dtype)


def _host(t):
    return t.detach().double().cpu().numpy()


def _inside(got, ref, e, u, what):
    got = _host(got) if torch.is_tensor(got) else got
    ratio = cases.within(got, ref, e, u)
    print("%s: max |err| / bound = %.3f (max |err| %.3e, max |ref| %.3e)" % (what, ratio.max(), np.abs(got - ref).max(), np.abs(ref).max()))
    assert np.isfinite(got).all() and ratio.max() <= 1.0, what


def _modules(ops, wdtype, pdtype, relu, affine, track, gpu, momentum=0.01, eps=cases.EPS):
    lin = nn.Linear(ops["cin"], ops["cout"], bias=False).to(gpu).to(wdtype)
    bn = nn.BatchNorm1d(ops["cout"], eps=eps, momentum=momentum, affine=affine, track_running_stats=track).to(gpu).to(pdtype)
    with torch.no_grad():
        lin.weight.copy_(_dev(ops["w"], wdtype, gpu))
        if affine:
            bn.weight.copy_(_dev(ops["gamma"], pdtype, gpu))
            bn.bias.copy_(_dev(ops["beta"], pdtype, gpu))
        if track:
            bn.running_mean.copy_(_dev(ops["rm"], pdtype, gpu))
            bn.running_var.copy_(_dev(ops["rv"], pdtype, gpu))
    return lin, bn, (nn.ReLU() if relu else None)


def _forward(mods, x):
    """Through linear_bn_relu16; fp32 rows (the exact case) through linear_bn_relu, the fp32 instance of the same kernel source."""
    op, node = (linear.linear_bn_relu, "_LinearBatchNormReLUBackward") if x.dtype == torch.float32 else (linear.linear_bn_relu16, NODE)
    y = op(mods[0], mods[1], x, mods[2])
    assert y is not None and y.dtype == x.dtype and type(y.grad_fn).__name__ == node
    saved = y.grad_fn.saved_tensors   # x, z, mean, invstd, w, gamma, beta
    assert saved[1].dtype == x.dtype and saved[2].dtype == saved[3].dtype == torch.float32
    return y, saved[1].clone(), saved[2].clone(), saved[3].clone()


def _three_stages(gpu, ops, dtype, wdtype, pdtype, relu, affine, track, mods=None, batch_stats=True, what=""):
    """Forward, the three stages, backward.  -> dict of the op's tensors (and the stage B references)."""
    n, cin, cout = ops["n"], ops["cin"], ops["cout"]
    u, up, uw = UNIT[dtype], UNIT[pdtype], UNIT[wdtype]
    if mods is None:
        mods = _modules(ops, wdtype, pdtype, relu, affine, track, gpu)
    lin, bn, _ = mods
    x = _dev(ops["x"], dtype, gpu).requires_grad_(True)
    y, z, mean, invstd = _forward(mods, x)
    z64 = _host(z)
    zr, e_z = cases.stage_a(ops["x"], ops["wt"])
    assert np.abs(z64).max() <= cases.Z_MAX
    _inside(z64, zr, e_z, u, what + " z")
    b = cases.stage_b(z64, ops["gamma"], ops["beta"], relu, ops["dy"], batch_stats=batch_stats, rm=ops["rm"], rv=ops["rv"])
    print("%s kink elements: %d of %d" % (what, b["kink"], n * cout))
    assert b["kink"] <= cases.KINK_FRACTION * n * cout
    _inside(y, b["y"], b["e"], u, what + " y")
    if batch_stats:
        assert (np.abs(_host(mean) - b["mean"]) <= b["e_mean"]).all(), what + " mean"
        assert (np.abs(_host(invstd) - b["invstd"]) <= b["e_invstd"]).all(), what + " invstd"
    if track and batch_stats:
        rm, rv, nbt, e_rm, e_rv = cases.running_step(z64, ops["rm"], ops["rv"], 0, bn.momentum, pdtype)
        assert bn.running_mean.dtype == pdtype and int(bn.num_batches_tracked.item()) == nbt == 1
        _inside(bn.running_mean, rm, e_rm, up, what + " running_mean")
        _inside(bn.running_var, rv, e_rv, up, what + " running_var")
    y.backward(_dev(b["dy"], dtype, gpu))
    dx64, e_dx, dw64, e_dw = cases.stage_c(b["du"], b["e_du"], ops["x"], ops["wt"], dtype)
    assert x.grad.dtype == dtype and lin.weight.grad.dtype == wdtype
    _inside(x.grad, dx64, e_dx, u, what + " dx")
    _inside(lin.weight.grad, dw64, e_dw, uw, what + " dw")
    if affine:
        assert bn.weight.grad.dtype == pdtype and bn.bias.grad.dtype == pdtype
        _inside(bn.weight.grad, b["dgamma"], b["e_dgamma"], up, what + " dgamma")
        _inside(bn.bias.grad, b["dbeta"], 0.0, up, what + " dbeta")
    return dict(y=y.detach(), z=z, dx=x.grad, dw=lin.weight.grad, mean=mean, invstd=invstd)


@pytest.mark.parametrize("n,cin,cout", cases.SHAPES)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_training_mode_three_stages(gpu, dtype, n, cin, cout):
    """Every shape class, uniform T parameters with ReLU + affine + tracked statistics, and fp32 BatchNorm parameters without any."""
    if (n, cin, cout) == cases.SPLIT_SHAPE:
        s = nat.call("fv2p_linear_bn_h_splits", n, cin, cout)
        assert s >= 3 and n % 128 != 0 and (s - 1) * 128 < n
    ops = cases.operands(n, cin, cout, dtype, dtype, dtype, True, 0)
    _three_stages(gpu, ops, dtype, dtype, dtype, True, True, True, what="uniform")
    ops = cases.operands(n, cin, cout, dtype, dtype, torch.float32, False, 1)
    _three_stages(gpu, ops, dtype, dtype, torch.float32, False, False, False, what="fp32 bn")


@pytest.mark.parametrize("n,cin,cout", cases.MASTER_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_master_weights_under_autocast(gpu, dtype, n, cin, cout):
    """An fp32 weight under autocast + set_mixed_precision(True): rounded once on its way into LDS, so y, dx and z carry the bits of the
    uniform route on w.to(T); dw is fp32, within the bound without the final 16-bit rounding."""
    ops = cases.operands(n, cin, cout, dtype, torch.float32, torch.float32, True, 2)
    before = spconv.mixed_precision()
    spconv.set_mixed_precision(True)
    try:
        with torch.autocast("cuda", dtype=dtype):
            master = _three_stages(gpu, ops, dtype, torch.float32, torch.float32, True, True, True, what="master")
    finally:
        spconv.set_mixed_precision(before)
    assert master["dw"].dtype == torch.float32
    uniform_ops = dict(ops, w=ops["wt"])
    uniform = _three_stages(gpu, uniform_ops, dtype, dtype, torch.float32, True, True, True, what="uniform")
    for k in ("y", "z", "dx"):
        assert torch.equal(master[k].view(torch.int16), uniform[k].view(torch.int16)), k


@pytest.mark.parametrize("n", [3, 65])
@pytest.mark.parametrize("momentum", [0.01, 1.0, None])
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_running_statistics(gpu, dtype, momentum, n):
    """torch's update on the op's z: the unbiased variance, the cumulative average for momentum=None (two calls), num_batches_tracked + 1
    per training call and none in eval mode; the float64 update rounded ONCE to the parameters' format after every step."""
    cin, cout = 5, 7
    for pdtype in (dtype, torch.float32):
        ops = cases.operands(n, cin, cout, dtype, dtype, pdtype, True, 3)
        mods = _modules(ops, dtype, pdtype, True, True, True, gpu, momentum=momentum)
        bn = mods[1]
        for call in range(2):
            rm0, rv0 = _host(bn.running_mean), _host(bn.running_var)
            x = _dev(cases.operands(n, cin, cout, dtype, dtype, pdtype, True, 30 + call)["x"], dtype, gpu).requires_grad_(True)
            _, z, _, _ = _forward(mods, x)
            rm, rv, nbt, e_rm, e_rv = cases.running_step(_host(z), rm0, rv0, call, momentum, pdtype)
            assert int(bn.num_batches_tracked.item()) == nbt == call + 1
            _inside(bn.running_mean, rm, e_rm, UNIT[pdtype], "running_mean call %d" % call)
            _inside(bn.running_var, rv, e_rv, UNIT[pdtype], "running_var call %d" % call)
        for m in mods:
            m.eval()
        kept = (bn.running_mean.clone(), bn.running_var.clone())
        assert linear.linear_bn_relu16(mods[0], bn, x.detach(), mods[2]) is not None
        assert int(bn.num_batches_tracked.item()) == 2
        assert torch.equal(bn.running_mean, kept[0]) and torch.equal(bn.running_var, kept[1])


@pytest.mark.parametrize("n,cin,cout", cases.EVAL_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_eval_mode(gpu, dtype, n, cin, cout):
    """One launch from the running statistics, and the backward pass through the frozen BatchNorm (batch_stats = 0)."""
    for pdtype in (dtype, torch.float32):
        ops = cases.operands(n, cin, cout, dtype, dtype, pdtype, True, 7)
        mods = [m.eval() for m in _modules(ops, dtype, pdtype, True, True, True, gpu)]
        _three_stages(gpu, ops, dtype, dtype, pdtype, True, True, True, mods=mods, batch_stats=False, what="eval")
        assert int(mods[1].num_batches_tracked.item()) == 0
        assert np.array_equal(_host(mods[1].running_mean), ops["rm"]) and np.array_equal(_host(mods[1].running_var), ops["rv"])


def test_eval_mode_without_grad_keeps_no_pre_activation(gpu):
    n, cin, cout = 64, 16, 16    # one n x cout tensor is 2048 bytes: a whole number of the allocator's blocks
    dtype = torch.float16
    ops = cases.operands(n, cin, cout, dtype, dtype, dtype, True, 8)
    lin, bn, relu = [m.eval() for m in _modules(ops, dtype, dtype, True, True, True, gpu)]
    x = _dev(ops["x"], dtype, gpu)
    with torch.no_grad():
        linear.linear_bn_relu16(lin, bn, x, relu)   # (the library is loaded, the allocator warm)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        y = linear.linear_bn_relu16(lin, bn, x, relu)
        after = torch.cuda.memory_allocated()
    assert y is not None and after - before == n * cout * 2, (before, after)
    before = torch.cuda.memory_allocated()
    y2 = linear.linear_bn_relu16(lin, bn, x, relu)    # a gradient can be asked for: y, z and the two [cout] vectors stay
    after = torch.cuda.memory_allocated()
    assert after - before >= 2 * n * cout * 2 and torch.equal(y, y2)


@pytest.mark.parametrize("n,cin,cout", [(130, 6, 20), (64, 32, 16)])
@pytest.mark.parametrize("dtype", DTYPES + [torch.float32], ids=dtype_id)
def test_exact_case_equals_the_oracle_bit_for_bit(gpu, dtype, n, cin, cout):
    """x in {-2, 2} balanced per column and one +-1 per weight row: z is a signed copy of a column, so mean = 0, var = 4, invstd = 0.5 with
    eps = 0 and integer gamma / beta give integer y.  Training-mode y, eval-mode y and the eval-mode dx (dz ternary, du a multiple of
    0.5) must equal the oracle bit for bit; dw too (integers below 256).  float32 rows (linear_bn_relu) are held to the same oracle
    values: the three formats of the one kernel source are pinned against each other.  Their eval route takes invstd from torch.rsqrt,
    which has to give exactly 0.5 for 4.0 on the device."""
    if dtype == torch.float32:
        assert torch.rsqrt(torch.full((cout,), 4.0, device=gpu)).eq(0.5).all(), "torch.rsqrt(4.0) on the device is not exactly 0.5"
    rng = np.random.default_rng(n + cin)
    x = np.stack([rng.permutation(np.repeat([-2.0, 2.0], n // 2)) for _ in range(cin)], axis=1)
    w = np.zeros((cout, cin))
    w[np.arange(cout), rng.integers(0, cin, cout)] = rng.integers(0, 2, cout) * 2.0 - 1.0
    gamma, beta = rng.integers(-2, 3, cout).astype(np.float64), rng.integers(-3, 4, cout).astype(np.float64)
    dy = ((rng.integers(0, 2, (n, cout)) * 2 - 1) * (rng.random((n, cout)) < 0.25)).astype(np.float64)
    z = x @ w.T
    for pdtype in dict.fromkeys((dtype, torch.float32)):
        ops = dict(n=n, cin=cin, cout=cout, w=w, gamma=gamma, beta=beta, rm=np.zeros(cout), rv=np.full(cout, 4.0))
        for training in (True, False):
            mods = _modules(ops, dtype, pdtype, True, True, True, gpu, eps=0.0)
            if not training:
                mods = [m.eval() for m in mods]
            xx = _dev(x, dtype, gpu).requires_grad_(True)
            y, zz, mean, invstd = _forward(mods, xx)
            pre, saved, _, _, _ = bn_oracle.bn_relu_forward(z, gamma, beta, np.zeros(cout), np.full(cout, 4.0), 0, False, None, 0.0, False)
            ref_y = np.maximum(pre, 0.0)
            assert np.array_equal(_host(zz), z) and np.array_equal(_host(y), ref_y), (training, "y")
            assert np.array_equal(_host(mean), np.zeros(cout)) and np.array_equal(_host(invstd), np.full(cout, 0.5))
            if not training:
                y.backward(_dev(dy, dtype, gpu))
                du, dgamma, dbeta = bn_oracle.bn_relu_backward(dy, ref_y, saved, gamma, True, False)
                ref_dw = du.T @ x
                assert np.abs(ref_dw).max() <= 256 and np.abs(dgamma).max() <= 256
                assert np.array_equal(_host(xx.grad), du @ w), "dx"
                assert np.array_equal(_host(mods[0].weight.grad), ref_dw), "dw"
                assert np.array_equal(_host(mods[1].weight.grad), dgamma) and np.array_equal(_host(mods[1].bias.grad), dbeta)


def _grads(gpu, ops, dtype, x_grad=True, w_grad=True):
    lin, bn, relu = _modules(ops, dtype, dtype, True, True, True, gpu)
    lin.weight.requires_grad_(w_grad)
    xx = _dev(ops["x"], dtype, gpu).requires_grad_(x_grad)
    y = linear.linear_bn_relu16(lin, bn, xx, relu)
    y.backward(_dev(ops["dy"], dtype, gpu))
    return {"y": y.detach(), "dx": xx.grad, "dw": lin.weight.grad, "dgamma": bn.weight.grad, "dbeta": bn.bias.grad,
            "running_mean": bn.running_mean, "running_var": bn.running_var}


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_needs_input_grad(gpu, dtype):
    ops = cases.operands(130, 6, 20, dtype, dtype, dtype, True, 9)
    full = _grads(gpu, ops, dtype)
    no_x = _grads(gpu, ops, dtype, x_grad=False)
    no_w = _grads(gpu, ops, dtype, w_grad=False)
    assert no_x["dx"] is None and no_w["dw"] is None and full["dx"] is not None and full["dw"] is not None
    for k in ("y", "dw", "dgamma", "dbeta"):
        assert torch.equal(no_x[k], full[k]), k
    for k in ("y", "dx", "dgamma", "dbeta"):
        assert torch.equal(no_w[k], full[k]), k


@pytest.mark.parametrize("n,cin,cout", cases.BITS_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_run_to_run_bits(gpu, dtype, n, cin, cout):
    """Forward + backward twice from identical copies of the modules, other allocator contents in between: the same bits."""
    ops = cases.operands(n, cin, cout, dtype, dtype, dtype, True, 10)
    a = _grads(gpu, ops, dtype)
    junk = torch.randn(1 << 20, device=gpu)   # other contents in the allocator's blocks between the two runs
    b = _grads(gpu, ops, dtype)
    del junk
    for k in a:
        assert torch.equal(a[k].view(torch.int16), b[k].view(torch.int16)), k


def test_declines(gpu):
    """Every situation that is not the plain one: None, and the modules' buffers untouched."""
    cin, cout, n = 6, 10, 9
    dtype = torch.float16
    x = torch.randn(n, cin, device=gpu).to(dtype)

    def mk(wdtype=dtype, pdtype=dtype):
        ops = cases.operands(n, cin, cout, dtype, wdtype, pdtype, True, 11)
        return list(_modules(ops, wdtype, pdtype, True, True, True, gpu))

    def declined(lin, bn, relu, xin):
        before = {k: v.clone() for k, v in bn.state_dict().items()}
        assert linear.fusable16(lin, bn, relu, xin) is False
        assert linear.linear_bn_relu16(lin, bn, xin, relu) is None
        for k, v in bn.state_dict().items():
            assert torch.equal(v, before[k]), k

    lin, bn, relu = mk()
    assert linear.fusable16(lin, bn, relu, x) is True
    assert linear.fusable16(lin, mk(pdtype=torch.float32)[1], relu, x) is True          # a BatchNorm kept in fp32
    declined(lin, bn, relu, x.float())                                                  # fp32 rows
    declined(lin, bn, relu, x.bfloat16())                                               # rows of the other 16-bit dtype
    mixed = mk()[1]
    mixed.running_mean = mixed.running_mean.float()
    mixed.running_var = mixed.running_var.float()
    declined(lin, mixed, relu, x)                                                       # mixed parameter dtypes
    declined(nn.Linear(cin, cout, bias=True).to(gpu).to(dtype), bn, relu, x)            # a Linear with bias

    class MyLinear(nn.Linear):
        pass
    declined(MyLinear(cin, cout, bias=False).to(gpu).to(dtype), bn, relu, x)            # a Linear subclass
    for which in range(3):                                                              # a hook on any of the three
        mods = mk()
        mods[which].register_forward_hook(lambda m, i, o: None)
        declined(*mods, x)
    for which in range(3):                                                              # forward replaced on the instance
        mods = mk()
        mods[which].forward = lambda t: t
        declined(*mods, x)
    declined(lin, bn, relu, torch.randn(cin, n, device=gpu).to(dtype).t())              # non-contiguous rows
    declined(mk(wdtype=torch.float32)[0], bn, relu, x)                                  # an fp32 weight outside autocast
    assert spconv.mixed_precision() is False
    with torch.autocast("cuda", dtype=dtype):
        declined(lin, bn, relu, x)                                                      # autocast without the mixed-precision switch
        declined(mk(wdtype=torch.float32)[0], bn, relu, x)
    declined(lin, bn, relu, x[:1])                                                      # one row in training mode: torch's error stays torch's
    ev = [m.eval() for m in mk()]
    assert linear.linear_bn_relu16(ev[0], ev[1], x[:1].contiguous(), ev[2]) is not None    # ... the same row in eval mode runs
    declined(lin, nn.BatchNorm1d(cout + 1).to(gpu).to(dtype), relu, x)                  # mismatched num_features
    saved = linear._ENABLED
    try:
        linear._ENABLED = False
        declined(lin, bn, relu, x)
    finally:
        linear._ENABLED = saved


def test_limits(gpu):
    """cin 1025 and cout 513: None from Python, FV2P_EINVAL from the C entry points - the shape and the dtypes are judged before any
    pointer is touched, with the entry point's name in the message."""
    dtype = torch.float16
    x = torch.randn(4, 1025, device=gpu).to(dtype)
    assert linear.linear_bn_relu16(nn.Linear(1025, 8, bias=False).to(gpu).to(dtype), nn.BatchNorm1d(8).to(gpu).to(dtype), x) is None
    x = torch.randn(4, 8, device=gpu).to(dtype)
    assert linear.linear_bn_relu16(nn.Linear(8, 513, bias=False).to(gpu).to(dtype), nn.BatchNorm1d(513).to(gpu).to(dtype), x) is None
    lib = nat.lib()

    def all_three(n, cin, cout, dt, wd, pd, word):
        rc = lib.fv2p_linear_bn_forward_h(None, n, cin, None, cout, 1e-3, 0.01, None, None, 1, None, None, None, None, None, None, None, dt, wd, pd, None, 0, None)
        assert rc == -1 and "fv2p_linear_bn_forward_h" in nat.last_error() and word in nat.last_error()
        rc = lib.fv2p_linear_bn_forward_eval_h(None, n, cin, None, cout, None, None, None, None, 1, None, None, dt, wd, pd, None)
        assert rc == -1 and "fv2p_linear_bn_forward_eval_h" in nat.last_error() and word in nat.last_error()
        rc = lib.fv2p_linear_bn_backward_h(None, None, None, n, cin, None, cout, None, None, None, None, 1, 1, None, None, None, None, None, dt, wd, pd, None, 0, None)
        assert rc == -1 and "fv2p_linear_bn_backward_h" in nat.last_error() and word in nat.last_error()

    for n, cin, cout in [(4, 1025, 8), (4, 8, 513), (4, 0, 8), (0, 8, 8)]:
        all_three(n, cin, cout, 1, 1, 1, "cin")
    for dt, wd, pd in [(0, 0, 0), (3, 3, 3), (1, 2, 1), (2, 2, 1)]:
        all_three(4, 8, 8, dt, wd, pd, "dtype")
    rc = lib.fv2p_linear_bn_forward_h(None, 1, 8, None, 8, 1e-3, 0.01, None, None, 1, None, None, None, None, None, None, None, 1, 1, 1, None, 0, None)   # n = 1
    assert rc == -1 and "fv2p_linear_bn_forward_h" in nat.last_error()


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


def _chain_check(names, hip, t16, f64, what):
    """rel_l2(hip, f64) <= max(K * rel_l2(torch16, f64), FLOOR): the op may be K times as far from float64 as torch's own 16-bit run."""
    bad = []
    for k in names:
        d_hip, d_ref = rel_l2(hip[k], f64[k]), rel_l2(t16[k], f64[k])
        print(f"{what} {k:13s} hip {d_hip:.2e}  torch16 {d_ref:.2e}  bound {max(K * d_ref, FLOOR):.2e}")
        if not d_hip <= max(K * d_ref, FLOOR):
            bad.append(f"{k}: {d_hip:.2e} from float64, the 16-bit torch run {d_ref:.2e}")
    assert not bad, (what, bad)


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_run_rows_on_a_lateral_block(gpu, monkeypatch, dtype):
    from fv2p_harness import fv2p_model
    torch.manual_seed(10)
    seq = nn.Sequential(nn.Linear(64, 192, bias=False), nn.BatchNorm1d(192, eps=1e-3, momentum=0.01), nn.ReLU(),
                        nn.Linear(192, 192, bias=False), nn.BatchNorm1d(192, eps=1e-3, momentum=0.01)).to(dtype)   # parameters of T values
    x = torch.randn(515, 64).to(dtype)
    dy = torch.randn(515, 192).to(dtype)
    plain = lambda s, t: s(t)
    f64, _ = _seq_grads(seq, x, dy, torch.float64, "cpu", plain)
    t16, _ = _seq_grads(seq, x, dy, dtype, gpu, plain)
    monkeypatch.setattr(linear, "pays16", lambda n, cin, cout, dt: True)
    for run in (linear.run_rows, fv2p_model.run_rows):
        hip, out = _seq_grads(seq, x, dy, dtype, gpu, run)
        assert out.dtype == dtype and _count_nodes(out.grad_fn, NODE) == 2
        _chain_check(list(f64), hip, t16, f64, run.__module__ + ".run_rows")
    monkeypatch.setattr(linear, "pays16", lambda n, cin, cout, dt: False)
    for run in (linear.run_rows, fv2p_model.run_rows):
        _, out = _seq_grads(seq, x, dy, dtype, gpu, run)
        assert _count_nodes(out.grad_fn, NODE) == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_bev_grid_pooling_compression(gpu, monkeypatch, dtype):
    from pcdet.models.backbones_3d.pfe import bev_grid_pooling as bgp
    torch.manual_seed(11)
    mod = bgp.BEVGridPooling(SimpleNamespace(IN_CHANNELS=16, OUT_CHANNELS=8), [0.0, -40.0, -3.0, 70.4, 40.0, 1.0], [0.05, 0.05, 0.1]).to(dtype)
    bev = torch.randn(2, 16, 25, 22, device=gpu).to(dtype)
    kp = torch.rand(2, 300, 3, device=gpu) * torch.tensor([8.0, 8.0, 1.0], device=gpu) + torch.tensor([0.0, -40.0, -2.0], device=gpu)
    dy = torch.randn(2, 300, 8).to(dtype)
    seq = mod.point_bev_feature_compress
    feats = mod.interpolate_from_bev_features(kp, bev, 2, 8).reshape(600, 16)
    assert feats.dtype == dtype
    plain = lambda s, t: s(t)
    f64, _ = _seq_grads(seq, feats.cpu(), dy.view(600, 8), torch.float64, "cpu", plain)
    t16, _ = _seq_grads(seq, feats, dy.view(600, 8), dtype, gpu, plain)
    monkeypatch.setattr(linear, "pays16", lambda n, cin, cout, dt: True)
    dev = copy.deepcopy(mod).to(gpu)
    out = dev({"spatial_features_before_head": bev, "spatial_features_stride": 8, "batch_size": 2}, kp)
    assert out.shape == (2, 300, 8) and out.dtype == dtype and _count_nodes(out.grad_fn, NODE) == 1
    out.backward(dy.to(gpu))
    hip = {"out": out.detach().view(600, 8)}
    hip.update({k: p.grad for k, p in dev.point_bev_feature_compress.named_parameters()})
    _chain_check(list(f64), hip, t16, f64, "BEVGridPooling")
