"""Cases of the 16-bit BatchNorm1d (+residual, +ReLU) tests (test_bn_half_cpu.py, test_bn_half_gpu.py).  Host only: operands and the
results of oracle/bn_oracle.py in float64 on operands ALREADY ROUNDED to the case's formats; every case is built once per process.

EXACT cases: x in {-2, +2} with exactly n/2 of each sign per channel (n even), eps = 0, gamma in {-2 .. 2}, beta and residual in
{-3 .. 3}.  Then mean = 0, var = 4 and invstd = 0.5 exactly, xhat = +-1 and y is an integer of magnitude <= 8: a kernel that works in
fp32 and stores 16 bits must reproduce the oracle BIT FOR BIT.  Running statistics move with a power-of-two momentum (or the
cumulative average), so that the oracle's float64 value is the same whichever way the product f * var * n / (n - 1) is associated; it
is then rounded ONCE to the parameters' format (`round64_to`).  The eval-mode backward (running_mean = 0, running_var = 4, ternary
dy with few non-zeros) is exact too: dx = gamma * 0.5 * dz, dgamma / dbeta are integers of magnitude <= 256.

RANDOM cases: standard-normal x times a per-channel scale in [0.5, 4] plus an offset in [-3, 3], rounded to the dtype; gamma in
[0.5, 1.5], beta in [-0.5, 0.5] rounded to the parameters' format; residual and dy standard normal, rounded.  Each case carries the
float64 results and the per-element error terms of the bound (see `fwd_error` / `bwd_error`)."""
import functools

import numpy as np
import torch

from oracle import bn_oracle
from half_cases import round_to

EPS24 = 2.0 ** -24
EXACT_MAX = 256
UNIT = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24}

# (n, c): the backbone's widths, multiples of 8 that are no multiple of 16 / 32, the element-wise path (20, 7), above 256 (vector path
# only) and the limit; rows: one reduce workgroup and several, ragged last blocks, more rows than one apply pass per thread (20 000 x 128)
EXACT_SHAPES = [(2, 16), (256, 32), (256, 24), (2050, 64), (20000, 128), (256, 40), (2050, 20), (256, 7), (258, 264), (256, 1024), (20000, 16)]
RANDOM_SHAPES = [(2, 16), (3, 32), (255, 64), (256, 128), (257, 24), (2049, 40), (20000, 128), (2049, 20), (255, 7), (257, 264), (255, 1024),
                 (20000, 16), (3, 7)]


def round64_to(a, dtype):
    """float64 array -> float64 array holding the values of `a` rounded to nearest even ONCE to the torch dtype (no intermediate fp32)."""
    a = np.asarray(a, np.float64)
    if dtype == torch.float32:
        return a.astype(np.float32).astype(np.float64)
    if dtype == torch.float16:
        return a.astype(np.float16).astype(np.float64)
    assert dtype == torch.bfloat16
    f = a.astype(np.float32)
    bits = f.view(np.uint32).copy()
    inexact = f.astype(np.float64) != a
    away = np.abs(f.astype(np.float64)) > np.abs(a)
    bits[inexact & away] -= 1            # towards zero, then the sticky bit: fp32 rounded to odd
    bits[inexact] |= 1
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & np.uint32(0xFFFF0000)
    return bits.view(np.float32).astype(np.float64)


def _seed(n, c, dtype, pdtype, tag):
    return (n * 1009 + c * 17 + (1 if dtype == torch.float16 else 2) * 5 + (0 if pdtype == torch.float32 else 3) + tag * 100003) % (2 ** 31)


@functools.lru_cache(maxsize=None)
def exact_case(n, c):
    """Operands are dtype-independent (small integers are exact in both formats).  -> dict with x, gamma, beta, res, dy and the
    oracle's float64 results: y[relu][has_res], bwd[relu][has_res] = (dx, dgamma, dbeta, dz)."""
    assert n % 2 == 0
    rng = np.random.default_rng(n * 31 + c)
    x = np.empty((n, c))
    half = np.repeat([-2.0, 2.0], n // 2)
    for j in range(c):
        x[:, j] = rng.permutation(half)
    gamma = rng.integers(-2, 3, size=c).astype(np.float64)
    beta = rng.integers(-3, 4, size=c).astype(np.float64)
    res = rng.integers(-3, 4, size=(n, c)).astype(np.float64)
    p = min(0.5, 200.0 / n)
    dy = (rng.integers(0, 2, size=(n, c)) * 2 - 1) * (rng.random((n, c)) < p)
    dy = dy.astype(np.float64)
    case = dict(n=n, c=c, x=x, gamma=gamma, beta=beta, res=res, dy=dy, y={}, bwd={})
    zeros, fours = np.zeros(c), np.full(c, 4.0)
    for relu in (False, True):
        for has_res in (False, True):
            # eval mode with running_mean = 0, running_var = 4 and training mode give the same y: the batch statistics ARE 0 and 4
            pre, saved, _, _, _ = bn_oracle.bn_relu_forward(x, gamma, beta, zeros, fours, 0, False, None, 0.0, False)
            tr, saved_t, _, _, _ = bn_oracle.bn_relu_forward(x, gamma, beta, None, None, 0, True, None, 0.0, False)
            assert np.array_equal(pre, tr) and np.array_equal(saved_t[0], zeros) and np.array_equal(saved_t[1], np.full(c, 0.5))
            if has_res:
                pre = pre + res
            y = np.maximum(pre, 0.0) if relu else pre
            dx, dgamma, dbeta = bn_oracle.bn_relu_backward(dy, y, saved, gamma, relu, False)
            dz = dy * ((y > 0) if relu else 1.0)
            case["y"][relu, has_res] = y
            case["bwd"][relu, has_res] = (dx, dgamma, dbeta, dz)
    return case


def exact_running(n, c, momentum, steps, pdtype):
    """Running statistics after `steps` training steps on an exact case, from (0, 1): the oracle's float64 update on the value
    rounded to the parameters' format after every step.  -> (running_mean, running_var, num_batches_tracked)"""
    case = exact_case(n, c)
    rm, rv, nbt = np.zeros(c), np.ones(c), 0
    for _ in range(steps):
        _, _, rm, rv, nbt = bn_oracle.bn_relu_forward(case["x"], case["gamma"], case["beta"], rm, rv, nbt, True, momentum, 0.0, False)
        rm, rv = round64_to(rm, pdtype), round64_to(rv, pdtype)
    return rm, rv, nbt


def fwd_error(x, mean, invstd, gamma, beta, res):
    """fp32 evaluation error of t = fl(fl(fl(fl(x - m) * s) * gamma) + beta) [+ res] with m = fl(mean), s = fl(invstd), u = 2^-24:
         m: |mean| u (+ one more |mean| u for the fp64 fold and division the statistic comes from: n 2^-53 << u)
         d = fl(x - m):          2 |mean| u + |x - mean| u          <= (|x| + 3 |mean|) u
         h = fl(d * s):          s (err d) + 2 |d| s u (s, product) <= s (3 |x| + 5 |mean|) u        =: exh
         p = fl(h * gamma):      |gamma| exh + |h gamma| u          <= |gamma| s (4 |x| + 6 |mean|) u
         t = fl(p + beta):       err p + |p + beta| u               <= [|gamma| s (5 |x| + 7 |mean|) + |beta|] u
         t = fl(t + res):        + (|t| + |res|) u                  <= + [|gamma| s (|x| + |mean|) + |beta| + |res|] u
       -> (e, exh); |x - mean| <= |x| + |mean| throughout, which more than covers the second-order terms."""
    ax, am, ag = np.abs(x), np.abs(mean), np.abs(gamma)
    exh = invstd * (3 * ax + 5 * am) * EPS24
    e = (ag * invstd * (5 * ax + 7 * am) + np.abs(beta)) * EPS24
    if res is not None:
        e = e + (ag * invstd * (ax + am) + np.abs(beta) + np.abs(res)) * EPS24
    return e, exh


def bwd_error(dz, xhat, exh, invstd, gamma, c1, c2, batch_stats):
    """fp32 evaluation error of dx = fl(fl(gamma * s) * fl(fl(dz - c1) - fl(h * c2))), h the kernel's xhat (error exh), u = 2^-24:
         c1 = fl32(sum dz / n): |c1| u;     c2 = fl32(sum dz h / n): |c2| u + mean(|dz| exh)   =: ec2   (the fp64 sums add nothing)
         A = fl(dz - c1):  |c1| u + |dz - c1| u                       <= (|dz| + 2 |c1|) u
         B = fl(h * c2):   exh |c2| + |xhat| ec2 + |xhat c2| u
         D = fl(A - B):    err A + err B + (|dz| + |c1| + |xhat c2|) u
         G = fl(gamma * s): 2 |gamma| s u;   dx = fl(G * D): |gamma| s (err D + 3 |D| u),  |D| <= |dz| + |c1| + |xhat c2|
       e_dx = |gamma| s [(5 |dz| + 6 |c1| + 5 |xhat c2|) u + exh |c2| + |xhat| ec2]
       dgamma = sum dz h: e = sum |dz| exh;  dbeta = sum dz: e = 0 (exact products, fp64 fold)   -> (e_dx, e_dgamma)"""
    adz, axh = np.abs(dz), np.abs(xhat)
    e_dgamma = (adz * exh).sum(0)
    if not batch_stats:
        c1, c2 = np.zeros_like(c1), np.zeros_like(c2)
    ec2 = (np.abs(c2) * EPS24 + (adz * exh).mean(0)) if batch_stats else np.zeros_like(c2)
    e_dx = np.abs(gamma) * invstd * ((5 * adz + 6 * np.abs(c1) + 5 * axh * np.abs(c2)) * EPS24 + exh * np.abs(c2) + axh * ec2)
    return e_dx, e_dgamma


@functools.lru_cache(maxsize=None)
def random_case(n, c, dtype, pdtype, relu, has_res, eps=1e-3):
    """Training-mode forward + backward.  float64 arrays holding values of `dtype` (x, res, dy) and of `pdtype` (gamma, beta)."""
    rng = np.random.default_rng(_seed(n, c, dtype, pdtype, 1 + 2 * relu + has_res))
    scale, offset = rng.uniform(0.5, 4.0, size=c), rng.uniform(-3.0, 3.0, size=c)
    x = round_to(rng.standard_normal((n, c)) * scale + offset, dtype)
    gamma, beta = round_to(rng.uniform(0.5, 1.5, size=c), pdtype), round_to(rng.uniform(-0.5, 0.5, size=c), pdtype)
    res = round_to(rng.standard_normal((n, c)), dtype) if has_res else None
    dy = round_to(rng.standard_normal((n, c)), dtype)

    def evaluate():
        pre, (mean, invstd, xhat), _, _, _ = bn_oracle.bn_relu_forward(x, gamma, beta, None, None, 0, True, None, eps, False)
        if has_res:
            pre = pre + res
        e, exh = fwd_error(x, mean, invstd, gamma, beta, res)
        return pre, mean, invstd, xhat, e, exh

    pre, mean, invstd, xhat, e, exh = evaluate()
    for _ in range(8):   # no pre-activation within the evaluation error (+ 2^-24: the smallest float16) of the ReLU's kink: redraw
        close = np.abs(pre) <= 4 * (e + EPS24)
        if not relu or not close.any():
            break
        x[close] = round_to(rng.standard_normal(int(close.sum())) * 2.0 + 1.0, dtype)
        pre, mean, invstd, xhat, e, exh = evaluate()
    y = np.maximum(pre, 0.0) if relu else pre
    dx, dgamma, dbeta = bn_oracle.bn_relu_backward(dy, y, (mean, invstd, xhat), gamma, relu, True)
    dz = dy * ((y > 0) if relu else 1.0)
    e_dx, e_dgamma = bwd_error(dz, xhat, exh, invstd, gamma, dz.mean(0), (dz * xhat).mean(0), True)
    return dict(n=n, c=c, x=x, gamma=gamma, beta=beta, res=res, dy=dy, eps=eps, pre=pre, y=y, mean=mean, invstd=invstd, dx=dx, dgamma=dgamma,
                dbeta=dbeta, dz=dz, e=e, e_dx=e_dx, e_dgamma=e_dgamma)


def random_case_ids():
    """(n, c, dtype, pdtype, relu, has_res) of every random case the GPU test runs: both dtypes and parameter formats on every shape,
    the four (relu, residual) forms spread over the shapes so that each shape sees two and each form every path."""
    ids = []
    for i, (n, c) in enumerate(RANDOM_SHAPES):
        for dtype in (torch.float16, torch.bfloat16):
            for pdtype in (torch.float32, dtype):
                forms = [(True, False), (True, True)] if i % 2 == 0 else [(False, True), (True, False)]
                if pdtype != torch.float32:
                    forms = forms[::-1][:1] + [(False, False)] if i % 3 == 0 else forms[:1]
                for relu, has_res in forms:
                    ids.append((n, c, dtype, pdtype, relu, has_res))
    return ids
