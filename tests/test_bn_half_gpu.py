"""GPU: BatchNorm1d (+residual, +ReLU) on float16 / bfloat16 rows (the Fmt16 instances of csrc/batchnorm.hip) through the raw C ABI, pcdet.ops.spconv.norm
and SparseSequential.  Cases and the float64 oracle results come from bn_half_cases.py (oracle/bn_oracle.py on rounded operands).

  1. exact cases: training forward (y, saved mean / invstd, running statistics after one and two steps, num_batches_tracked), eval
     forward and eval backward (dx, dgamma, dbeta, dz_out) equal the oracle bit for bit;
  2. random cases, forward and training backward: |got - ref64| <= u (|ref64| + e) + e + 2^-24 element-wise, nothing measured in it:
       u = 2^-11 (float16) / 2^-8 (bfloat16) / 2^-24 (an fp32 parameter gradient): ONE rounding of the result to its format;
       e: the fp32 evaluation error of the kernel's own expression, derived term by term in bn_half_cases.fwd_error / bwd_error:
            y:  [|gamma| s (5 |x| + 7 |mean|) + |beta|] 2^-24   (+ [|gamma| s (|x| + |mean|) + |beta| + |res|] 2^-24 with a residual)
            dx: |gamma| s [(5 |dz| + 6 |c1| + 5 |xhat c2|) 2^-24 + exh |c2| + |xhat| ec2],  exh = s (3 |x| + 5 |mean|) 2^-24 the error
                of the kernel's xhat, ec2 = |c2| 2^-24 + mean(|dz| exh) that of c2
            dgamma: sum |dz| exh;  dbeta: 0 (exact terms folded in fp64: only the final rounding);
       2^-24: float16 results below 2^-14 are subnormal and round with an absolute error;
  3. conv -> BatchNorm1d -> ReLU through SparseSequential after .half() / .bfloat16(), and with the BatchNorm kept in fp32;
  4. no fp32 copy: the peak memory of forward + backward stays below the fp32 copies of x and dy alone;
  5. two runs are bit-identical;  6. argument checks leave the outputs untouched;  7. what the route declines."""
import numpy as np
import pytest
import torch
from torch import nn

import bn_half_cases as cases
import fv2p_native as nat
import half_cases
import pcdet.ops.spconv as spconv
from oracle import bn_oracle
from pcdet.ops.spconv import norm

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]
DT_CODE = {torch.float16: 1, torch.bfloat16: 2}
UNIT = cases.UNIT
dtype_id = lambda d: str(d).replace("torch.", "")
FORMS = [(False, False), (True, False), (False, True), (True, True)]   # (relu, residual)
FILL = 77.0


def _dev(a, dtype, gpu):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(gpu).to(dtype)


def _host(t):
    return t.detach().double().cpu().numpy()


def _pd(dtype, pdtype):
    return 0 if pdtype == torch.float32 else DT_CODE[dtype]


def _ws(c, gpu):
    return nat.workspace(nat.lib().fv2p_batchnorm_h_ws_bytes(0, c), gpu)


def _p(t):
    return 0 if t is None else t.data_ptr()


def raw_forward(x, gamma, beta, relu, res, rm, rv, nbt, eps, momentum, dtype, pdtype, gpu, code=None, pd=None, ws_bytes=None, n=None):
    nn_, c = x.shape
    mean, invstd = (torch.full((c,), FILL, dtype=torch.float32, device=gpu) for _ in range(2))
    y = torch.full_like(x, FILL)
    ws = _ws(c, gpu)
    rc = nat.lib().fv2p_batchnorm_forward_h(_p(x), nn_ if n is None else n, c, eps, -1.0 if momentum is None else momentum, _p(gamma), _p(beta), int(relu),
                                            _p(res), _p(rm), _p(rv), _p(nbt), _p(mean), _p(invstd), _p(y), DT_CODE[dtype] if code is None else code,
                                            _pd(dtype, pdtype) if pd is None else pd, _p(ws), ws.numel() if ws_bytes is None else ws_bytes, nat.stream())
    return rc, y, mean, invstd


def raw_backward(x, dy, mean, invstd, gamma, beta, relu, batch_stats, mask_y, want_dz, dtype, pdtype, gpu, code=None, pd=None, ws_bytes=None, n=None):
    nn_, c = x.shape
    dx = torch.full_like(x, FILL)
    dz = torch.full_like(x, FILL) if want_dz else None
    dgamma, dbeta = (torch.full((c,), FILL, dtype=pdtype, device=gpu) for _ in range(2))
    ws = _ws(c, gpu)
    rc = nat.lib().fv2p_batchnorm_backward_h(_p(x), _p(dy), nn_ if n is None else n, c, _p(mean), _p(invstd), _p(gamma), _p(beta), int(relu), int(batch_stats),
                                             _p(mask_y), _p(dx), _p(dz), _p(dgamma), _p(dbeta), DT_CODE[dtype] if code is None else code,
                                             _pd(dtype, pdtype) if pd is None else pd, _p(ws), ws.numel() if ws_bytes is None else ws_bytes, nat.stream())
    return rc, dx, dz, dgamma, dbeta


def _same(got, ref, what):
    assert np.array_equal(_host(got), ref), what


@pytest.mark.parametrize("n,c", cases.EXACT_SHAPES)
@pytest.mark.parametrize("pkind", ["fp32", "same"])
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_exact_cases_equal_the_oracle_bit_for_bit(gpu, dtype, pkind, n, c):
    pdtype = torch.float32 if pkind == "fp32" else dtype
    case = cases.exact_case(n, c)
    x, res, dy = (_dev(case[k], dtype, gpu) for k in ("x", "res", "dy"))
    gamma, beta = _dev(case["gamma"], pdtype, gpu), _dev(case["beta"], pdtype, gpu)
    zeros, half_ = np.zeros(c), np.full(c, 0.5)
    # momentum = None (the cumulative average: every channel reads num_batches_tracked before workgroup 0 advances it) where c spans
    # more than one wave of channels, a power of two elsewhere
    momentum = None if c in (128, 264) else 0.25
    for relu, has_res in FORMS:
        ref_y = case["y"][relu, has_res]
        rm, rv = torch.zeros(c, dtype=pdtype, device=gpu), torch.ones(c, dtype=pdtype, device=gpu)
        nbt = torch.zeros((), dtype=torch.int64, device=gpu)
        for step in (1, 2):
            rc, y, mean, invstd = raw_forward(x, gamma, beta, relu, res if has_res else None, rm, rv, nbt, 0.0, momentum, dtype, pdtype, gpu)
            assert rc == 0, nat.last_error()
            _same(y, ref_y, ("training y", relu, has_res, step))
            _same(mean, zeros, "saved mean")
            _same(invstd, half_, "saved invstd")
            ref_rm, ref_rv, ref_nbt = cases.exact_running(n, c, momentum, step, pdtype)
            _same(rm, ref_rm, ("running_mean", step))
            _same(rv, ref_rv, ("running_var", step))
            assert int(nbt.item()) == ref_nbt == step
        # eval mode: running_mean = 0, running_var = 4, eps = 0 -> mean 0, invstd 0.5
        mean_t, invstd_t = torch.zeros(c, device=gpu), torch.full((c,), 0.5, device=gpu)
        y = torch.full_like(x, FILL)
        nat.call("fv2p_batchnorm_apply_h", x, n, c, mean_t, invstd_t, gamma, beta, int(relu), res if has_res else None, y, DT_CODE[dtype],
                 _pd(dtype, pdtype), nat.stream())
        _same(y, ref_y, ("eval y", relu, has_res))
        ref_dx, ref_dgamma, ref_dbeta, ref_dz = case["bwd"][relu, has_res]
        mask_y = y if (has_res and relu) else None      # the residual form reads its mask from the block's output
        rc, dx, dz, dgamma, dbeta = raw_backward(x, dy, mean_t, invstd_t, gamma, beta, relu, False, mask_y, has_res, dtype, pdtype, gpu)
        assert rc == 0, nat.last_error()
        _same(dx, ref_dx, ("eval dx", relu, has_res))
        _same(dgamma, ref_dgamma, "eval dgamma")
        _same(dbeta, ref_dbeta, "eval dbeta")
        if has_res:
            _same(dz, ref_dz, "dz_out")


def _assert_within(got, ref, e, u, what):
    """|got - ref| <= u (|ref| + e) + e + 2^-24 element-wise; prints the largest ratio before it asserts."""
    got = _host(got)
    bound = u * (np.abs(ref) + e) + e + 2.0 ** -24
    ratio = np.abs(got - ref) / bound
    print("%s: max |err| / bound = %.3f (max |err| %.3e, max |ref| %.3e)" % (what, ratio.max(), np.abs(got - ref).max(), np.abs(ref).max()))
    assert np.isfinite(got).all() and ratio.max() <= 1.0, what


def _module(c, pdtype, gamma, beta, gpu, eps=1e-3, momentum=0.01):
    bn = nn.BatchNorm1d(c, eps=eps, momentum=momentum).to(gpu).to(pdtype)
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    return bn


def run_op(case, dtype, pdtype, relu, has_res, gpu):
    """Training forward + backward through norm.batch_norm_relu -> (y, dx, dres, dgamma, dbeta, bn)."""
    c = case["c"]
    bn = _module(c, pdtype, _dev(case["gamma"], pdtype, gpu), _dev(case["beta"], pdtype, gpu), gpu, eps=case["eps"])
    x = _dev(case["x"], dtype, gpu).requires_grad_(True)
    res = _dev(case["res"], dtype, gpu).requires_grad_(True) if has_res else None
    y = norm.batch_norm_relu(bn, x, nn.ReLU() if relu else None, residual=res)
    assert y is not None and y.dtype == dtype and y.grad_fn.name() == "_BatchNormReLU16Backward"
    y.backward(_dev(case["dy"], dtype, gpu))
    assert x.grad.dtype == dtype and bn.weight.grad.dtype == pdtype and bn.bias.grad.dtype == pdtype
    assert res is None or res.grad.dtype == dtype
    return y, x.grad, None if res is None else res.grad, bn.weight.grad, bn.bias.grad, bn


@pytest.mark.parametrize("args", cases.random_case_ids(), ids=lambda a: "-".join(str(v).replace("torch.", "") for v in a))
def test_random_cases_within_the_derived_bound(gpu, args):
    n, c, dtype, pdtype, relu, has_res = args
    case = cases.random_case(*args)
    y, dx, dres, dgamma, dbeta, bn = run_op(case, dtype, pdtype, relu, has_res, gpu)
    u, up = UNIT[dtype], UNIT[pdtype]
    _assert_within(y, case["y"], case["e"], u, "y")
    _assert_within(dx, case["dx"], case["e_dx"], u, "dx")
    _assert_within(dgamma, case["dgamma"], case["e_dgamma"], up, "dgamma")
    _assert_within(dbeta, case["dbeta"], 0.0, up, "dbeta")
    if has_res:   # dz = dy or 0: no rounding at all
        assert np.array_equal(_host(dres), case["dz"])
    assert int(bn.num_batches_tracked.item()) == 1
    # saved statistics: the fp64 statistic (fold error n 2^-53, far below) rounded to fp32 once; two roundings allowed
    rc, _, mean, invstd = raw_forward(_dev(case["x"], dtype, gpu), None, None, False, None, None, None, None, case["eps"], 0.01, dtype, pdtype, gpu)
    assert rc == 0, nat.last_error()
    assert (np.abs(_host(mean) - case["mean"]) <= 2 * 2.0 ** -24 * np.abs(case["mean"])).all()
    assert (np.abs(_host(invstd) - case["invstd"]) <= 2 * 2.0 ** -24 * case["invstd"]).all()


@pytest.mark.parametrize("bn_fp32", [False, True], ids=["bn16", "bn32"])
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_conv_batchnorm_relu_block_through_sparse_sequential(gpu, dtype, bn_fp32):
    """The conv's own result (checked against its float64 oracle with the conv test's bound) is what the BatchNorm reads; the block's
    output is then compared with bn_oracle on exactly those 16-bit rows.  Gradients: dtypes, and dgamma / dbeta within the bound, where
    a pre-activation within e of the ReLU's kink may fall on either side (its |dy| (|xhat|) is added to the allowance)."""
    cin, cout = 32, 64
    case = half_cases.random_case("subm", cin, cout, dtype)
    pdtype = torch.float32 if bn_fp32 else dtype
    net = spconv.SparseSequential(spconv.SubMConv3d(cin, cout, 3, padding=1, bias=False, indice_key="k"),
                                  nn.BatchNorm1d(cout, eps=1e-3, momentum=0.01), nn.ReLU()).to(gpu).to(dtype)
    if bn_fp32:
        net[1].float()
    rng = np.random.default_rng(5)
    gamma, beta = cases.round_to(rng.uniform(0.5, 1.5, cout), pdtype), cases.round_to(rng.uniform(-0.5, 0.5, cout), pdtype)
    with torch.no_grad():
        net[0].weight.copy_(_dev(case["w"], dtype, gpu))
        net[1].weight.copy_(_dev(gamma, pdtype, gpu))
        net[1].bias.copy_(_dev(beta, pdtype, gpu))
    ind = torch.from_numpy(case["ind"]).to(gpu)
    feats = _dev(case["feats"], dtype, gpu).requires_grad_(True)
    with torch.no_grad():
        h = net[0](spconv.SparseConvTensor(feats.detach(), ind, case["shape"], case["batch"])).features
    assert h.dtype == dtype
    u = UNIT[dtype]
    e_conv = case["n_ref"] * 2.0 ** -24 * case["s_ref"]
    _assert_within(h, case["ref"], e_conv, u, "conv")
    out = net(spconv.SparseConvTensor(feats, ind, case["shape"], case["batch"]))
    y = out.features
    assert y.dtype == dtype and y.grad_fn.name() == "_BatchNormReLU16Backward"      # the 16-bit route was taken
    h64 = _host(h)
    n = h64.shape[0]
    pre, (mean, invstd, xhat), rm, rv, nbt = bn_oracle.bn_relu_forward(h64, gamma, beta, np.zeros(cout), np.ones(cout), 0, True, float(np.float32(0.01)), 1e-3, False)   # the momentum the kernel is handed: a float
    e, exh = cases.fwd_error(h64, mean, invstd, gamma, beta, None)
    _assert_within(y, np.maximum(pre, 0.0), e, u, "block output")
    up = UNIT[pdtype]
    _assert_within(net[1].running_mean, rm, 0.0, up, "running_mean")
    _assert_within(net[1].running_var, rv, 0.0, up, "running_var")
    assert int(net[1].num_batches_tracked.item()) == nbt == 1 and net[1].running_mean.dtype == pdtype
    dy = cases.round_to(rng.standard_normal((n, cout)), dtype)
    y.backward(_dev(dy, dtype, gpu))
    assert feats.grad.dtype == dtype and net[0].weight.grad.dtype == dtype and net[1].weight.grad.dtype == pdtype and net[1].bias.grad.dtype == pdtype
    assert all(bool(torch.isfinite(t).all()) for t in (feats.grad, net[0].weight.grad, net[1].weight.grad, net[1].bias.grad))
    dz = dy * (pre > 0)
    near = np.abs(pre) <= e + 2.0 ** -24
    _assert_within(net[1].weight.grad, (dz * xhat).sum(0), (np.abs(dz) * exh).sum(0) + (near * np.abs(dy * xhat)).sum(0), up, "dgamma")
    _assert_within(net[1].bias.grad, dz.sum(0), (near * np.abs(dy)).sum(0), up, "dbeta")


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_no_fp32_copy_of_x_or_dy_is_made(gpu, dtype):
    """A route through fp32 kernels holds fp32 copies of x and dy (8 n c bytes) before it allocates any result.  The 16-bit op allocates
    y and dx (4 n c bytes) and [C]-sized statistics."""
    n, c = 20000, 128
    case = cases.random_case(n, c, dtype, dtype, True, False)
    bn = _module(c, dtype, _dev(case["gamma"], dtype, gpu), _dev(case["beta"], dtype, gpu), gpu)
    x, dy = _dev(case["x"], dtype, gpu).requires_grad_(True), _dev(case["dy"], dtype, gpu)
    relu = nn.ReLU()

    def step():
        y = norm.batch_norm_relu(bn, x, relu)
        assert y is not None and y.dtype == dtype
        y.backward(dy)
        assert x.grad.dtype == dtype
        x.grad = None
        bn.zero_grad(set_to_none=True)

    step()   # the grow-only workspace exists from here on
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print("peak %d bytes; 16-bit results %d; fp32 copies of x and dy %d" % (peak, 4 * n * c, 8 * n * c))
    assert peak < 8 * n * c


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_two_runs_are_bit_identical(gpu, dtype):
    args = (20000, 128, dtype, dtype, True, True)
    case = cases.random_case(*args)
    a = run_op(case, *args[2:], gpu)[:5]
    b = run_op(case, *args[2:], gpu)[:5]
    for p, q in zip(a, b):
        assert torch.equal(p.view(torch.int16), q.view(torch.int16))


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_argument_checks_leave_the_outputs_untouched(gpu, dtype):
    case = cases.exact_case(256, 32)
    n, c = 256, 32
    x, dy = _dev(case["x"], dtype, gpu), _dev(case["dy"], dtype, gpu)
    gamma, beta = _dev(case["gamma"], dtype, gpu), _dev(case["beta"], dtype, gpu)
    mean_t, invstd_t = torch.zeros(c, device=gpu), torch.full((c,), 0.5, device=gpu)
    other = 3 - DT_CODE[dtype]
    bad = [dict(code=0), dict(code=3), dict(code=-1), dict(pd=other), dict(pd=7), dict(ws_bytes=8), dict(n=0)]
    for kw in bad:
        rc, y, mean, invstd = raw_forward(x, gamma, beta, True, None, None, None, None, 0.0, 0.25, dtype, dtype, gpu, **kw)
        assert (rc == 0) if "n" in kw else (rc < 0), kw
        if "code" in kw:
            assert "dtype" in nat.last_error()
        rc2, dx, dz, dgamma, dbeta = raw_backward(x, dy, mean_t, invstd_t, gamma, beta, True, True, None, True, dtype, dtype, gpu, **kw)
        assert (rc2 == 0) if "n" in kw else (rc2 < 0), kw
        torch.cuda.synchronize()
        for t in (y, mean, invstd, dx, dz, dgamma, dbeta):
            assert bool((t == FILL).all()), kw
    y = torch.full_like(x, FILL)
    lib = nat.lib()
    for code, pd, nn_ in ((0, 0, n), (DT_CODE[dtype], other, n), (DT_CODE[dtype], 0, 0)):
        rc = lib.fv2p_batchnorm_apply_h(_p(x), nn_, c, _p(mean_t), _p(invstd_t), 0, 0, 1, 0, _p(y), code, pd, nat.stream())
        assert (rc == 0) if nn_ == 0 else (rc < 0)
    # c beyond the limits: 1032 on the vector path, 264 + 1 on the element-wise one
    wide = torch.zeros((4, 1032), dtype=dtype, device=gpu)
    assert lib.fv2p_batchnorm_apply_h(_p(wide), 4, 1032, _p(mean_t), _p(invstd_t), 0, 0, 1, 0, _p(wide), DT_CODE[dtype], 0, nat.stream()) == -4
    assert lib.fv2p_batchnorm_apply_h(_p(wide), 4, 265, _p(mean_t), _p(invstd_t), 0, 0, 1, 0, _p(wide), DT_CODE[dtype], 0, nat.stream()) == -4
    torch.cuda.synchronize()
    assert bool((y == FILL).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_what_the_16_bit_route_declines(gpu, dtype):
    c = 16
    bn = nn.BatchNorm1d(c, eps=1e-3, momentum=0.01).to(gpu).to(dtype)
    x = torch.randn(8, c, device=gpu).to(dtype)
    assert norm.batch_norm_relu(bn, x, nn.ReLU()) is not None
    assert norm.batch_norm_relu(bn, x[:1], nn.ReLU()) is None                      # one row in training mode: torch raises there
    bn.eval()
    assert norm.batch_norm_relu(bn, x[:1], nn.ReLU()) is not None                  # ... but not in eval mode
    bn.train()
    with torch.autocast("cuda", dtype=dtype):
        assert norm.batch_norm_relu(bn, x, nn.ReLU()) is None
    hooked = nn.BatchNorm1d(c).to(gpu).to(dtype)
    hooked.register_forward_hook(lambda m, i, o: None)
    assert norm.batch_norm_relu(hooked, x, nn.ReLU()) is None
    relu = nn.ReLU()
    relu.register_forward_hook(lambda m, i, o: None)
    assert norm.batch_norm_relu(bn, x, relu) is None
    mixed = nn.BatchNorm1d(c).to(gpu).to(dtype)
    mixed.weight.data = mixed.weight.data.float()                                  # parameters neither all fp32 nor all of x's dtype
    assert norm.batch_norm_relu(mixed, x, None) is None
    assert norm.batch_norm_relu(bn, x.t().contiguous().t(), None) is None          # not contiguous
    assert norm.batch_norm_relu(nn.BatchNorm1d(c + 1).to(gpu).to(dtype), x, None) is None
    assert norm.batch_norm_relu(bn, x, None, residual=x.float()) is None           # a residual of another dtype
    assert not norm.fusable(bn, None, x, c)                                        # the fp32 predicate keeps its meaning


def _bits(t):
    return t.view({torch.float32: torch.int32, torch.int64: torch.int64}.get(t.dtype, torch.int16))


def _cross_format_call(x32, dy32, res32, gamma, beta, dtype):
    """Training forward (ReLU, tracked statistics, momentum None from num_batches_tracked 3), the eval-style apply with a residual on
    that call's mean / invstd, then backward with batch_stats = 0 and relu = 0, through the raw C ABI with fp32 parameters: the fp32
    entry points (forward, apply_res, backward) for torch.float32, the _h ones (param_dtype 0) otherwise."""
    n, c = x32.shape
    gpu = x32.device
    x, dy, res = x32.to(dtype), dy32.to(dtype), res32.to(dtype)
    assert all(torch.equal(a.float(), b) for a, b in ((x, x32), (dy, dy32), (res, res32)))   # the grid is exact in the format
    mean, invstd, dgamma, dbeta = (torch.full((c,), FILL, device=gpu) for _ in range(4))
    rm, rv = torch.linspace(-1.0, 1.0, c, device=gpu), torch.linspace(0.5, 2.0, c, device=gpu)
    nbt = torch.full((), 3, dtype=torch.int64, device=gpu)
    y, y_res, dx = (torch.full_like(x, FILL) for _ in range(3))
    s = nat.stream()
    if dtype == torch.float32:
        ws = nat.workspace(nat.call("fv2p_batchnorm_ws_bytes", n, c), gpu)
        nat.call("fv2p_batchnorm_forward", x, n, c, 1e-3, -1.0, gamma, beta, 1, rm, rv, nbt, mean, invstd, y, ws, ws.numel(), s)
        nat.call("fv2p_batchnorm_apply_res", x, n, c, mean, invstd, gamma, beta, 1, res, y_res, s)
        nat.call("fv2p_batchnorm_backward", x, dy, n, c, mean, invstd, gamma, beta, 0, 0, dx, dgamma, dbeta, ws, ws.numel(), s)
    else:
        ws, code = _ws(c, gpu), DT_CODE[dtype]
        nat.call("fv2p_batchnorm_forward_h", x, n, c, 1e-3, -1.0, gamma, beta, 1, None, rm, rv, nbt, mean, invstd, y, code, 0, ws, ws.numel(), s)
        nat.call("fv2p_batchnorm_apply_h", x, n, c, mean, invstd, gamma, beta, 1, res, y_res, code, 0, s)
        nat.call("fv2p_batchnorm_backward_h", x, dy, n, c, mean, invstd, gamma, beta, 0, 0, None, dx, None, dgamma, dbeta, code, 0, ws, ws.numel(), s)
    torch.cuda.synchronize()
    return dict(mean=mean, invstd=invstd, running_mean=rm, running_var=rv, num_batches_tracked=nbt, dbeta=dbeta, y=y, y_res=y_res, dx=dx)


@pytest.mark.parametrize("shape", [(37, 5), (700, 12), (700, 24)], ids=lambda s: "x".join(str(v) for v in s))
def test_the_three_formats_agree_bit_for_bit_on_values_all_of_them_hold(gpu, shape):
    """x, dy and the residual on the grid k / 8, |k| <= 64: exact in fp32, float16 and bfloat16 (7 significant bits).  Their sums and sums
    of squares are multiples of 1 / 64 far below 2^53 units: exact in fp64 in any order, so the different geometries of the width-4 and
    width-8 reductions cannot show.  (37, 5) takes the element path in every format; (700, 12) the vector path in fp32 and the element
    path in 16 bits; (700, 24) the vector path everywhere, on 3 partials in fp32 and 2 in 16 bits.  The statistics are then the same fp64
    values (momentum None: the factor 1 / 4 from num_batches_tracked 3), y the same fp32 expression rounded once, and with
    batch_stats = 0 and relu = 0 (c1 = c2 = 0, no mask: float16 underflow cannot enter) so is dx; dbeta is the exact sum of dy.  dgamma
    is left out: its terms dy * xhat are not exact.  Nothing is a tolerance."""
    n, c = shape
    rng = np.random.default_rng(n * 1009 + c * 17)
    grid = lambda: torch.from_numpy(rng.integers(-64, 65, size=shape).astype(np.float32) / 8).to(gpu)
    x32, dy32, res32 = grid(), grid(), grid()
    gamma = torch.from_numpy(rng.uniform(0.5, 1.5, size=c).astype(np.float32)).to(gpu)
    beta = torch.from_numpy(rng.uniform(-0.75, 0.75, size=c).astype(np.float32)).to(gpu)
    ref = _cross_format_call(x32, dy32, res32, gamma, beta, torch.float32)
    assert int(ref["num_batches_tracked"].item()) == 4 and not any(bool((ref[k] == FILL).any()) for k in ("y", "y_res", "dx"))
    for dtype in DTYPES:
        got = _cross_format_call(x32, dy32, res32, gamma, beta, dtype)
        for k in ("mean", "invstd", "running_mean", "running_var", "num_batches_tracked", "dbeta"):
            assert torch.equal(_bits(got[k]), _bits(ref[k])), (dtype, k)
        for k in ("y", "y_res", "dx"):
            assert got[k].dtype == dtype and torch.equal(_bits(got[k]), _bits(ref[k].to(dtype))), (dtype, k)
