"""GPU: BatchNorm2d (+ReLU) on float16 / bfloat16 NCHW maps (the 16-bit instances of csrc/batchnorm2d.hip) through the raw C ABI and through
pcdet.ops.spconv.norm.batch_norm2d_relu16.  A map [n, c, hw] is the rows [n * hw, c] of bn_half_cases.py by a permutation, so its exact
cases, `round64_to`, `UNIT`, `fwd_error` and `bwd_error` apply as they are: the kernel's expressions are the ones whose error terms those
functions derive term by term.

  1. exact cases (integers, mean 0, invstd 0.5, eps 0): training y, saved mean / invstd, running statistics after one and two steps,
     num_batches_tracked, eval y and eval dx / dgamma / dbeta equal the float64 oracle bit for bit;
  2. random cases, training forward and backward: |got - ref64| <= u (|ref64| + e) + e + 2^-24 element-wise, u from UNIT (ONE rounding
     of the result to its format), e from fwd_error / bwd_error, 2^-24 for float16 subnormals.  Nothing in it is measured.  The backward
     reference takes the kernel's own mask (stored y > 0), which may differ from the float64 mask in at most 0.1 % of the elements; the
     data (per-channel std 0.5 - 2, |beta| in 0.25 - 0.75, fixed seeds) keep a host evaluation of the same fp32 expression inside
     that cap, which is asserted as well;
  3. float16 underflow: positive pre-activations below 2^-25 are stored as zeros and get zero dx;
  4. the option matrix (affine, tracking, momentum, train / eval, ReLU) by the same bound;
  5. two runs are bit-identical;  6. a non-contiguous dz gives the bits of its contiguous copy;  7. no fp32 copy of x or dz;
  8. argument checks leave the outputs untouched;  9. what the route declines;
  10. on values that fp32, float16 and bfloat16 all hold, the three formats' kernels give the same bits (one kernel source)."""
import functools
import itertools

import numpy as np
import pytest
import torch
from torch import nn

import bn_half_cases as cases
import fv2p_native as nat
import pcdet.ops.spconv as spconv
from half_cases import round_to
from oracle import bn_oracle
from pcdet.ops.spconv import norm

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]
DT_CODE = {torch.float16: 1, torch.bfloat16: 2}
UNIT = cases.UNIT
C16 = norm.BN2D_CHUNK16
FILL = 77.0
MASK_CAP = 1e-3
dtype_id = lambda d: str(d).replace("torch.", "")

# (n, c, h, w, offset): offset = the maps live one element into their buffers (hw % 8 == 0, pointer not 16-byte aligned: element path)
SHAPES = [(2, 3, 5, 7, 0),            # element path, misaligned planes
          (3, 8, 4, 4, 0),            # vector path, one chunk
          (2, 4, 2, 6, 0),            # hw = 12: divisible by 4, not by 8: element path
          (1, 1, 1, 2, 0),            # smallest training batch
          (2, 5, 1, C16 + 1, 0),      # chunk border, element path, last chunk of one element
          (2, 4, 1, C16 + 8, 0),      # chunk border, vector path, last chunk of one 16-byte unit
          (300, 2, 1, 2, 0),          # 300 partials per channel: more than one round of the fold
          (2, 1, 4, 4, 0), (2, 64, 4, 4, 0), (2, 65, 4, 4, 0), (2, 256, 4, 4, 0), (2, 257, 4, 4, 0),
          (3, 8, 4, 4, 1)]
shape_id = lambda s: "x".join(str(v) for v in s[:4]) + ("+1" if s[4] else "")
MATRIX_SHAPES = [(2, 3, 5, 7, 0), (2, 4, 1, C16 + 8, 0)]


def to_map(rows, n, c, hw):
    """rows [n * hw, c] -> map [n, c, hw] (numpy)"""
    return np.ascontiguousarray(rows.reshape(n, hw, c).transpose(0, 2, 1))


def to_rows(t, n, c, hw):
    """map tensor [n, c, h, w] -> float64 rows [n * hw, c] on the host"""
    return t.detach().double().cpu().numpy().reshape(n, c, hw).transpose(0, 2, 1).reshape(n * hw, c)


def _place(a, dtype, gpu, shape, offset):
    """float64 array -> tensor of `shape` on the GPU, `offset` elements into its buffer"""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(gpu).to(dtype).reshape(shape)
    if not offset:
        return t
    buf = torch.empty(t.numel() + offset, dtype=dtype, device=gpu)
    v = buf[offset:].view(shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


def _filled(like, offset):
    buf = torch.full((like.numel() + offset,), FILL, dtype=like.dtype, device=like.device)
    return buf[offset:].view(like.shape)


def _vec(a, dtype, gpu):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(gpu).to(dtype)


def _host(t):
    return t.detach().double().cpu().numpy()


def _p(t):
    return 0 if t is None else t.data_ptr()


def _pd(dtype, pdtype):
    return 0 if pdtype == torch.float32 else DT_CODE[dtype]


def _ws(n, c, hw, gpu):
    return nat.workspace(nat.call("fv2p_batchnorm2d_h_ws_bytes", n, c, hw), gpu)


def raw_forward(x, gamma, beta, relu, rm, rv, nbt, eps, momentum, dtype, pdtype, offset=0, code=None, pd=None, ws_bytes=None, null=False):
    n, c, h, w = x.shape
    gpu = x.device
    mean, invstd = (torch.full((c,), FILL, dtype=torch.float32, device=gpu) for _ in range(2))
    y = _filled(x, offset)
    ws = _ws(n, c, h * w, gpu)
    rc = nat.lib().fv2p_batchnorm2d_forward_h(0 if null else _p(x), n, c, h * w, eps, -1.0 if momentum is None else momentum, _p(gamma), _p(beta),
                                              int(relu), _p(rm), _p(rv), _p(nbt), _p(mean), _p(invstd), _p(y), DT_CODE[dtype] if code is None else code,
                                              _pd(dtype, pdtype) if pd is None else pd, _p(ws), ws.numel() if ws_bytes is None else ws_bytes, nat.stream())
    return rc, y, mean, invstd


def raw_apply(x, mean, invstd, gamma, beta, relu, dtype, pdtype, offset=0, code=None, pd=None, null=False):
    n, c, h, w = x.shape
    y = _filled(x, offset)
    rc = nat.lib().fv2p_batchnorm2d_apply_h(0 if null else _p(x), n, c, h * w, _p(mean), _p(invstd), _p(gamma), _p(beta), int(relu), _p(y),
                                            DT_CODE[dtype] if code is None else code, _pd(dtype, pdtype) if pd is None else pd, nat.stream())
    return rc, y


def raw_backward(x, dz, mean, invstd, gamma, beta, relu, batch_stats, dtype, pdtype, offset=0, code=None, pd=None, ws_bytes=None, null=False):
    n, c, h, w = x.shape
    gpu = x.device
    dx = _filled(x, offset)
    dgamma, dbeta = (torch.full((c,), FILL, dtype=pdtype, device=gpu) for _ in range(2))
    ws = _ws(n, c, h * w, gpu)
    rc = nat.lib().fv2p_batchnorm2d_backward_h(0 if null else _p(x), _p(dz), n, c, h * w, _p(mean), _p(invstd), _p(gamma), _p(beta), int(relu),
                                               int(batch_stats), _p(dx), _p(dgamma), _p(dbeta), DT_CODE[dtype] if code is None else code,
                                               _pd(dtype, pdtype) if pd is None else pd, _p(ws), ws.numel() if ws_bytes is None else ws_bytes, nat.stream())
    return rc, dx, dgamma, dbeta


# ---- 1. exact cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
@pytest.mark.parametrize("pkind", ["fp32", "same"])
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_exact_cases_equal_the_oracle_bit_for_bit(gpu, dtype, pkind, shape):
    n, c, h, w, offset = shape
    hw, rows = h * w, n * h * w
    pdtype = torch.float32 if pkind == "fp32" else dtype
    case = cases.exact_case(rows, c)
    x = _place(to_map(case["x"], n, c, hw), dtype, gpu, (n, c, h, w), offset)
    dz = _place(to_map(case["dy"], n, c, hw), dtype, gpu, (n, c, h, w), offset)
    gamma, beta = _vec(case["gamma"], pdtype, gpu), _vec(case["beta"], pdtype, gpu)
    zeros, half_ = np.zeros(c), np.full(c, 0.5)
    momentum = None if c > 64 else 0.25   # the cumulative average: every channel reads the count before channel 0's workgroup advances it
    same = lambda got, ref, what: np.testing.assert_array_equal(to_rows(got, n, c, hw), ref, err_msg=str(what))
    for relu in (False, True):
        ref_y = case["y"][relu, False]
        rm, rv = torch.zeros(c, dtype=pdtype, device=gpu), torch.ones(c, dtype=pdtype, device=gpu)
        nbt = torch.zeros((), dtype=torch.int64, device=gpu)
        for step in (1, 2):
            rc, y, mean, invstd = raw_forward(x, gamma, beta, relu, rm, rv, nbt, 0.0, momentum, dtype, pdtype, offset)
            assert rc == 0, nat.last_error()
            same(y, ref_y, ("training y", relu, step))
            assert np.array_equal(_host(mean), zeros) and np.array_equal(_host(invstd), half_)
            ref_rm, ref_rv, ref_nbt = cases.exact_running(rows, c, momentum, step, pdtype)
            assert np.array_equal(_host(rm), ref_rm), ("running_mean", step)
            assert np.array_equal(_host(rv), ref_rv), ("running_var", step)
            assert int(nbt.item()) == ref_nbt == step
        # eval mode: running_mean = 0, running_var = 4, eps = 0 -> mean 0, invstd 0.5
        mean_t, invstd_t = torch.zeros(c, device=gpu), torch.full((c,), 0.5, device=gpu)
        rc, y = raw_apply(x, mean_t, invstd_t, gamma, beta, relu, dtype, pdtype, offset)
        assert rc == 0, nat.last_error()
        same(y, ref_y, ("eval y", relu))
        ref_dx, ref_dgamma, ref_dbeta, _ = case["bwd"][relu, False]
        rc, dx, dgamma, dbeta = raw_backward(x, dz, mean_t, invstd_t, gamma, beta, relu, False, dtype, pdtype, offset)
        assert rc == 0, nat.last_error()
        same(dx, ref_dx, ("eval dx", relu))
        assert np.array_equal(_host(dgamma), ref_dgamma) and np.array_equal(_host(dbeta), ref_dbeta)


# ---- 2. / 4. random cases ------------------------------------------------------------------------------------------------------------
def stored_positive_fp32(x, mean, invstd, gamma, beta, dtype):
    """The mask a host evaluation of the kernel's fp32 expression gives on the same 16-bit operands: round(t) > 0."""
    f = np.float32
    t = ((x.astype(f) - mean.astype(f)) * invstd.astype(f)) * gamma.astype(f) + beta.astype(f)
    return round_to(t.astype(np.float64), dtype) > 0


@functools.lru_cache(maxsize=None)
def random_case(shape, dtype, pdtype, affine=True, track=True, momentum=0.01, training=True, relu=True, eps=1e-3):
    """Host only.  Rows [n * hw, c] in float64 holding values of the formats; the float64 forward and its error terms."""
    n, c, h, w, _ = shape
    rows = n * h * w
    seed = (rows * 1009 + c * 17 + DT_CODE[dtype] * 5 + (0 if pdtype == torch.float32 else 3) + 7 * affine + 11 * track + 13 * training + 19 * relu
            + (0 if momentum is None else 23))
    rng = np.random.default_rng(seed)
    scale, offset = rng.uniform(0.5, 2.0, size=c), rng.uniform(-3.0, 3.0, size=c)
    x = round_to(rng.standard_normal((rows, c)) * scale + offset, dtype)
    dz = round_to(rng.standard_normal((rows, c)), dtype)
    if affine:
        gamma = round_to(rng.uniform(0.5, 1.5, size=c), pdtype)
        beta = round_to(rng.uniform(0.25, 0.75, size=c) * rng.choice([-1.0, 1.0], size=c), pdtype)
    else:
        gamma, beta = np.ones(c), np.zeros(c)
    rm = round_to(offset + rng.uniform(-0.2, 0.2, size=c), pdtype) if track else None
    rv = round_to(scale ** 2 * rng.uniform(0.8, 1.25, size=c), pdtype) if track else None
    nbt = 3
    batch_stats = training or not track
    pre, (mean, invstd, xhat), new_rm, new_rv, new_nbt = bn_oracle.bn_relu_forward(x, gamma, beta, rm, rv, nbt, training, momentum, eps, False)
    e, exh = cases.fwd_error(x, mean, invstd, gamma, beta, None)
    mask64 = pre > 0
    host_mask = stored_positive_fp32(x, mean, invstd, gamma, beta, dtype)
    assert (host_mask != mask64).mean() <= MASK_CAP, "the data do not keep the fp32 expression's mask inside the cap"
    return dict(shape=shape, x=x, dz=dz, gamma=gamma, beta=beta, rm=rm, rv=rv, nbt=nbt, batch_stats=batch_stats, pre=pre, mean=mean, invstd=invstd,
                xhat=xhat, e=e, exh=exh, mask64=mask64, new_rm=new_rm, new_rv=new_rv, new_nbt=new_nbt, affine=affine, track=track, momentum=momentum,
                training=training, relu=relu, eps=eps)


def _module(case, pdtype, gpu):
    c = case["shape"][1]
    bn = nn.BatchNorm2d(c, eps=case["eps"], momentum=case["momentum"], affine=case["affine"], track_running_stats=case["track"]).to(gpu).to(pdtype)
    with torch.no_grad():
        if case["affine"]:
            bn.weight.copy_(_vec(case["gamma"], pdtype, gpu))
            bn.bias.copy_(_vec(case["beta"], pdtype, gpu))
        if case["track"]:
            bn.running_mean.copy_(_vec(case["rm"], pdtype, gpu))
            bn.running_var.copy_(_vec(case["rv"], pdtype, gpu))
            bn.num_batches_tracked.fill_(case["nbt"])
    return bn.train(case["training"])


def run_op(case, dtype, pdtype, gpu, dz=None):
    """Forward + backward through norm.batch_norm2d_relu16 -> (y, dx, dgamma, dbeta, bn)."""
    n, c, h, w, offset = case["shape"]
    bn = _module(case, pdtype, gpu)
    x = _place(to_map(case["x"], n, c, h * w), dtype, gpu, (n, c, h, w), offset).detach().requires_grad_(True)
    assert norm.batch_norm2d_relu(bn, x, nn.ReLU() if case["relu"] else None) is None      # the fp32 op keeps declining
    y = norm.batch_norm2d_relu16(bn, x, nn.ReLU() if case["relu"] else None)
    assert y is not None and y.dtype == dtype and y.shape == x.shape and y.grad_fn.name() == "_BatchNorm2dReLU16Backward"
    y.backward(_place(to_map(case["dz"], n, c, h * w), dtype, gpu, (n, c, h, w), offset) if dz is None else dz)
    assert x.grad.dtype == dtype
    if case["affine"]:
        assert bn.weight.grad.dtype == pdtype and bn.bias.grad.dtype == pdtype
    return y, x.grad, bn.weight.grad if case["affine"] else None, bn.bias.grad if case["affine"] else None, bn


def _assert_within(got, ref, e, u, what):
    """|got - ref| <= u (|ref| + e) + e + 2^-24 element-wise; prints the largest ratio before it asserts."""
    bound = u * (np.abs(ref) + e) + e + 2.0 ** -24
    ratio = np.abs(got - ref) / bound
    print("%s: max |err| / bound = %.3f (max |err| %.3e, max |ref| %.3e)" % (what, ratio.max(), np.abs(got - ref).max(), np.abs(ref).max()))
    assert np.isfinite(got).all() and ratio.max() <= 1.0, what


def check_case(case, dtype, pdtype, gpu):
    n, c, h, w, _ = case["shape"]
    hw = h * w
    u, up = UNIT[dtype], UNIT[pdtype]
    y, dx, dgamma, dbeta, bn = run_op(case, dtype, pdtype, gpu)
    relu, batch_stats = case["relu"], case["batch_stats"]
    got_y = to_rows(y, n, c, hw)
    _assert_within(got_y, np.maximum(case["pre"], 0.0) if relu else case["pre"], case["e"], u, "y")
    # the backward reference takes the kernel's own mask: the stored y > 0
    mask = (got_y > 0) if relu else np.ones_like(case["mask64"])
    if relu:
        differ = (mask != case["mask64"]).mean()
        print("mask differs from the float64 mask in %.4f %% of the elements" % (100 * differ))
        assert differ <= MASK_CAP
    saved = (case["mean"], case["invstd"], case["xhat"])
    ref_dx, ref_dgamma, ref_dbeta = bn_oracle.bn_relu_backward(case["dz"], mask.astype(np.float64), saved, case["gamma"], relu, batch_stats)
    dzm = case["dz"] * mask
    e_dx, e_dgamma = cases.bwd_error(dzm, case["xhat"], case["exh"], case["invstd"], case["gamma"], dzm.mean(0), (dzm * case["xhat"]).mean(0), batch_stats)
    _assert_within(to_rows(dx, n, c, hw), ref_dx, e_dx, u, "dx")
    if case["affine"]:
        _assert_within(_host(dgamma), ref_dgamma, e_dgamma, up, "dgamma")
        _assert_within(_host(dbeta), ref_dbeta, 0.0, up, "dbeta")
    if case["track"]:
        # fp64 statistics (the fold differs from numpy's by n 2^-53) rounded ONCE to the parameters' format
        for got, ref, what in ((bn.running_mean, case["new_rm"], "running_mean"), (bn.running_var, case["new_rv"], "running_var")):
            assert (np.abs(_host(got) - ref) <= up * np.abs(ref) * (1 + 2.0 ** -20) + 2.0 ** -40).all(), what
        assert int(bn.num_batches_tracked.item()) == case["new_nbt"]


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
@pytest.mark.parametrize("pkind", ["fp32", "same"])
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_random_cases_within_the_derived_bound(gpu, dtype, pkind, shape):
    pdtype = torch.float32 if pkind == "fp32" else dtype
    case = random_case(shape, dtype, pdtype)
    check_case(case, dtype, pdtype, gpu)
    # saved statistics through the raw ABI: the fp64 statistic rounded to fp32 once; two roundings allowed
    n, c, h, w, offset = shape
    x = _place(to_map(case["x"], n, c, h * w), dtype, gpu, (n, c, h, w), offset)
    rc, _, mean, invstd = raw_forward(x, None, None, False, None, None, None, case["eps"], 0.01, dtype, pdtype, offset)
    assert rc == 0, nat.last_error()
    assert (np.abs(_host(mean) - case["mean"]) <= 2 * 2.0 ** -24 * np.abs(case["mean"]) + 2.0 ** -40).all()
    assert (np.abs(_host(invstd) - case["invstd"]) <= 2 * 2.0 ** -24 * case["invstd"]).all()


@pytest.mark.parametrize("shape", MATRIX_SHAPES, ids=shape_id)
@pytest.mark.parametrize("pkind", ["fp32", "same"])
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_option_matrix(gpu, dtype, pkind, shape):
    pdtype = torch.float32 if pkind == "fp32" else dtype
    for affine, track, momentum, training, relu in itertools.product((True, False), (True, False), (0.01, None), (True, False), (True, False)):
        print("affine %s tracking %s momentum %s training %s relu %s" % (affine, track, momentum, training, relu))
        check_case(random_case(shape, dtype, pdtype, affine, track, momentum, training, relu), dtype, pdtype, gpu)


# ---- 3. float16 underflow ------------------------------------------------------------------------------------------------------------
def test_float16_preactivations_below_the_smallest_subnormal_get_no_gradient(gpu):
    """Channel 0: t = x * 2^-13 with x in {1, 2, 3} * 2^-14, so 0 < t <= 3 * 2^-27 < 2^-25: stored as 0, and dx = 0 although the fp32 t is
    positive.  Channel 1 has beta = 1: stored positive, dx = invstd * dz = 0.125."""
    dtype = torch.float16
    n, c, h, w = 2, 2, 4, 4
    k = torch.arange(n * h * w, device=gpu).view(n, 1, h, w) % 3 + 1
    x = (k.double() * 2.0 ** -14).to(dtype).expand(n, c, h, w).contiguous()
    dz = torch.full_like(x, 1024.0)
    mean_t, invstd_t = torch.zeros(c, device=gpu), torch.full((c,), 2.0 ** -13, device=gpu)
    gamma, beta = torch.ones(c, device=gpu), torch.tensor([0.0, 1.0], device=gpu)
    rc, y = raw_apply(x, mean_t, invstd_t, gamma, beta, True, dtype, torch.float32)
    assert rc == 0, nat.last_error()
    assert bool((y[:, 0] == 0).all()) and bool((y[:, 1] == 1).all())
    rc, dx, dgamma, dbeta = raw_backward(x, dz, mean_t, invstd_t, gamma, beta, True, False, dtype, torch.float32)
    assert rc == 0, nat.last_error()
    assert bool((dx[:, 0] == 0).all()) and bool((dx[:, 1] == 0.125).all())
    assert float(dgamma[0]) == 0.0 and float(dbeta[0]) == 0.0 and float(dbeta[1]) == 1024.0 * n * h * w
    # without the ReLU the same elements do get their gradient
    rc, dx, _, _ = raw_backward(x, dz, mean_t, invstd_t, gamma, beta, False, False, dtype, torch.float32)
    assert rc == 0 and bool((dx == 0.125).all())


# ---- 5. / 6. / 7. --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 5, 1, C16 + 1, 0), (2, 4, 1, C16 + 8, 0), (300, 2, 1, 2, 0)], ids=shape_id)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_two_runs_are_bit_identical(gpu, dtype, shape):
    case = random_case(shape, dtype, dtype)
    a, b = run_op(case, dtype, dtype, gpu), run_op(case, dtype, dtype, gpu)
    for p, q in zip(a[:4], b[:4]):
        assert torch.equal(p.view(torch.int16), q.view(torch.int16))
    for p, q in zip(a[4].state_dict().values(), b[4].state_dict().values()):
        assert torch.equal(p, q)


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_a_non_contiguous_gradient_gives_the_bits_of_its_contiguous_copy(gpu, dtype):
    shape = (3, 8, 4, 4, 0)
    case = random_case(shape, dtype, dtype)
    wide = torch.randn(3, 8, 4, 8, device=gpu).to(dtype)
    dz = wide[..., ::2]
    assert not dz.is_contiguous()
    a, b = run_op(case, dtype, dtype, gpu, dz=dz), run_op(case, dtype, dtype, gpu, dz=dz.contiguous())
    for p, q in zip(a[1:4], b[1:4]):
        assert torch.equal(p.view(torch.int16), q.view(torch.int16))


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_no_fp32_copy_of_x_or_dz_is_made(gpu, dtype):
    """A route through fp32 kernels holds fp32 copies of x and dz (8 bytes per element) before it allocates any result.  The 16-bit op
    allocates y and dx (4 bytes per element) and [C]-sized statistics."""
    n, c, h, w = 2, 16, 64, 64
    numel = n * c * h * w
    bn = nn.BatchNorm2d(c, eps=1e-3, momentum=0.01).to(gpu).to(dtype)
    x, dz = torch.randn(n, c, h, w, device=gpu).to(dtype).requires_grad_(True), torch.randn(n, c, h, w, device=gpu).to(dtype)
    relu = nn.ReLU()

    def step():
        y = norm.batch_norm2d_relu16(bn, x, relu)
        assert y is not None and y.dtype == dtype
        y.backward(dz)
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
    print("peak %d bytes; 16-bit results %d; fp32 copies of x and dz %d" % (peak, 4 * numel, 8 * numel))
    assert peak < 8 * numel


# ---- 8. argument checks --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_argument_checks_leave_the_outputs_untouched(gpu, dtype):
    n, c, h, w = 3, 8, 4, 4
    case = cases.exact_case(n * h * w, c)
    x = _place(to_map(case["x"], n, c, h * w), dtype, gpu, (n, c, h, w), 0)
    dz = _place(to_map(case["dy"], n, c, h * w), dtype, gpu, (n, c, h, w), 0)
    gamma, beta = _vec(case["gamma"], dtype, gpu), _vec(case["beta"], dtype, gpu)
    mean_t, invstd_t = torch.zeros(c, device=gpu), torch.full((c,), 0.5, device=gpu)
    other = 3 - DT_CODE[dtype]
    bad = [(dict(code=0), -1), (dict(code=3), -1), (dict(code=-1), -1), (dict(pd=other), -1), (dict(pd=7), -1), (dict(null=True), -1),
           (dict(ws_bytes=8), -2)]
    for kw, want in bad:
        rm, rv = torch.full((c,), FILL, dtype=dtype, device=gpu), torch.full((c,), FILL, dtype=dtype, device=gpu)
        nbt = torch.full((), 5, dtype=torch.int64, device=gpu)
        rc, y, mean, invstd = raw_forward(x, gamma, beta, True, rm, rv, nbt, 0.0, 0.25, dtype, dtype, **kw)
        assert rc == want, (kw, nat.last_error())
        if "code" in kw or "pd" in kw:
            assert "dtype" in nat.last_error()
        rc2, dx, dgamma, dbeta = raw_backward(x, dz, mean_t, invstd_t, gamma, beta, True, True, dtype, dtype, **kw)
        assert rc2 == want, (kw, nat.last_error())
        outs = [y, mean, invstd, rm, rv, dx, dgamma, dbeta]
        if "ws_bytes" not in kw:
            rc3, y2 = raw_apply(x, mean_t, invstd_t, gamma, beta, True, dtype, dtype, **kw)
            assert rc3 == want, (kw, nat.last_error())
            outs.append(y2)
        torch.cuda.synchronize()
        for t in outs:
            assert bool((t == FILL).all()), kw
        assert int(nbt.item()) == 5
    lib = nat.lib()
    y = torch.full_like(x, FILL)
    assert lib.fv2p_batchnorm2d_apply_h(_p(x), 0, c, h * w, _p(mean_t), _p(invstd_t), 0, 0, 1, _p(y), DT_CODE[dtype], 0, nat.stream()) == 0   # n == 0
    assert lib.fv2p_batchnorm2d_apply_h(_p(x), 1 << 20, 1 << 10, 1, _p(mean_t), _p(invstd_t), 0, 0, 1, _p(y), DT_CODE[dtype], 0, nat.stream()) == -4
    torch.cuda.synchronize()
    assert bool((y == FILL).all())


# ---- 9. declines ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_what_the_16_bit_route_declines(gpu, dtype):
    c = 8
    bn = nn.BatchNorm2d(c, eps=1e-3, momentum=0.01).to(gpu).to(dtype)
    relu = nn.ReLU()
    x = torch.randn(2, c, 4, 4, device=gpu).to(dtype)
    assert norm.batch_norm2d_relu16(bn, x, relu) is not None
    assert norm.batch_norm2d_relu(bn, x, relu) is None and not norm.fusable2d(bn, relu, x)     # the fp32 op and its predicate keep their meaning
    assert norm.batch_norm2d_relu16(nn.BatchNorm2d(c).to(gpu), x, relu) is not None            # parameters kept in fp32
    assert norm.batch_norm2d_relu16(nn.BatchNorm2d(c).to(gpu), x.float(), relu) is None        # an fp32 map is the other op's
    hooked = nn.BatchNorm2d(c).to(gpu).to(dtype)
    hooked.register_forward_hook(lambda m, i, o: None)
    assert norm.batch_norm2d_relu16(hooked, x, relu) is None
    patched = nn.BatchNorm2d(c).to(gpu).to(dtype)
    patched.forward = lambda t: t
    assert norm.batch_norm2d_relu16(patched, x, relu) is None
    hrelu = nn.ReLU()
    hrelu.register_forward_hook(lambda m, i, o: None)
    assert norm.batch_norm2d_relu16(bn, x, hrelu) is None
    assert norm.batch_norm2d_relu16(bn, x.contiguous(memory_format=torch.channels_last), relu) is None
    assert norm.batch_norm2d_relu16(bn, torch.randn(2, c, 4, 8, device=gpu).to(dtype)[..., ::2], relu) is None     # strided
    assert norm.batch_norm2d_relu16(bn, x[:1, :, :1, :1], relu) is None                          # one value per channel in training mode
    bn.eval()
    assert norm.batch_norm2d_relu16(bn, x[:1, :, :1, :1].contiguous(), relu) is not None         # ... but not in eval mode
    bn.train()
    nobias = nn.BatchNorm2d(c).to(gpu).to(dtype)
    nobias.bias = None
    assert norm.batch_norm2d_relu16(nobias, x, relu) is None                                     # weight without bias
    mixed = nn.BatchNorm2d(c).to(gpu).to(dtype)
    mixed.weight.data = mixed.weight.data.float()                                                # neither all fp32 nor all of x's dtype
    assert norm.batch_norm2d_relu16(mixed, x, relu) is None
    other = nn.BatchNorm2d(c).to(gpu).to(torch.bfloat16 if dtype == torch.float16 else torch.float16)
    assert norm.batch_norm2d_relu16(other, x, relu) is None
    assert norm.batch_norm2d_relu16(nn.BatchNorm2d(c).to(dtype), x, relu) is None                # parameters not on the GPU
    assert norm.batch_norm2d_relu16(nn.BatchNorm2d(c + 1).to(gpu).to(dtype), x, relu) is None
    with torch.autocast("cuda", dtype=dtype):
        assert norm.batch_norm2d_relu16(bn, x, relu) is None                                     # autocast ...
        spconv.set_mixed_precision(True)
        try:
            y = norm.batch_norm2d_relu16(bn, x, relu)                                            # ... unless the 16-bit route was asked for
            assert y is not None and y.dtype == dtype
        finally:
            spconv.set_mixed_precision(False)


# ---- 10. the three formats agree -----------------------------------------------------------------------------------------------------
def _bits(t):
    return t.view({torch.float32: torch.int32, torch.int64: torch.int64}.get(t.dtype, torch.int16))


def _cross_format_call(x32, dz32, gamma, beta, dtype):
    """Training forward (ReLU, tracked statistics), then backward with batch_stats = 0 and relu = 0 on that call's mean / invstd, through
    the raw C ABI with fp32 parameters (param_dtype 0): the fp32 entry points for torch.float32, the _h ones otherwise."""
    n, c, h, w = x32.shape
    hw, gpu = h * w, x32.device
    sfx, fmt = ("", ()) if dtype == torch.float32 else ("_h", (DT_CODE[dtype], 0))
    x, dz = x32.to(dtype), dz32.to(dtype)
    assert torch.equal(x.float(), x32) and torch.equal(dz.float(), dz32)   # the grid is exact in the format
    mean, invstd, dgamma, dbeta = (torch.full((c,), FILL, device=gpu) for _ in range(4))
    rm, rv = torch.linspace(-1.0, 1.0, c, device=gpu), torch.linspace(0.5, 2.0, c, device=gpu)
    nbt = torch.full((), 3, dtype=torch.int64, device=gpu)
    y, dx = torch.full_like(x, FILL), torch.full_like(x, FILL)
    ws = nat.workspace(nat.call("fv2p_batchnorm2d%s_ws_bytes" % sfx, n, c, hw), gpu)
    nat.call("fv2p_batchnorm2d_forward" + sfx, x, n, c, hw, 1e-3, 0.01, gamma, beta, 1, rm, rv, nbt, mean, invstd, y, *fmt, ws, ws.numel(), nat.stream())
    nat.call("fv2p_batchnorm2d_backward" + sfx, x, dz, n, c, hw, mean, invstd, gamma, beta, 0, 0, dx, dgamma, dbeta, *fmt, ws, ws.numel(),
             nat.stream())
    torch.cuda.synchronize()
    return dict(mean=mean, invstd=invstd, running_mean=rm, running_var=rv, num_batches_tracked=nbt, dbeta=dbeta, y=y, dx=dx)


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (2, 4, 1, C16 + 8)], ids=lambda s: "x".join(str(v) for v in s))
def test_the_three_formats_agree_bit_for_bit_on_values_all_of_them_hold(gpu, shape):
    """x and dz on the grid k / 8, |k| <= 64: exact in fp32, float16 and bfloat16 (7 significant bits).  Their sums and sums of squares
    are multiples of 1 / 64 below 2^36 units: exact in fp64 in any order, so the per-thread orders of the width-4 and width-8 kernels
    cannot show.  (2, 3, 5, 7) takes the element path in every format, (2, 4, 1, chunk + 8) the vector path with two chunks per plane
    and a short tail.  The statistics are then the same fp64 values, y the same fp32 expression rounded once, and with batch_stats = 0
    and relu = 0 (c1 = c2 = 0, no mask: float16 underflow cannot enter) so is dx; dbeta is the exact sum of dz.  Nothing is a tolerance."""
    n, c, h, w = shape
    rng = np.random.default_rng(n * 1009 + c * 17 + h * w)
    grid = lambda: torch.from_numpy(rng.integers(-64, 65, size=shape).astype(np.float32) / 8).to(gpu)
    x32, dz32 = grid(), grid()
    gamma = torch.from_numpy(rng.uniform(0.5, 1.5, size=c).astype(np.float32)).to(gpu)
    beta = torch.from_numpy(rng.uniform(-0.75, 0.75, size=c).astype(np.float32)).to(gpu)
    ref = _cross_format_call(x32, dz32, gamma, beta, torch.float32)
    assert int(ref["num_batches_tracked"].item()) == 4 and not bool((ref["y"] == FILL).any())
    for dtype in DTYPES:
        got = _cross_format_call(x32, dz32, gamma, beta, dtype)
        for k in ("mean", "invstd", "running_mean", "running_var", "num_batches_tracked", "dbeta"):
            assert torch.equal(_bits(got[k]), _bits(ref[k])), (dtype, k)
        for k in ("y", "dx"):
            assert got[k].dtype == dtype and torch.equal(_bits(got[k]), _bits(ref[k].to(dtype))), (dtype, k)
