"""Cases of the 16-bit Linear + BatchNorm1d (+ReLU) tests (test_linear_bn_half_cpu.py, test_linear_bn_half_gpu.py).  Host only, not a
test module: operands ALREADY ROUNDED to the case's formats, references = the arithmetic contract of csrc/linear_bn.hip's 16-bit formats in float64,
and bounds derived from the number formats alone - nothing in here is measured.

T is float16 or bfloat16, u = 2^-11 / 2^-8 its unit roundoff; an fp32 accumulation costs 2^-24 per addition; 2^-24 absolute covers the
float16 subnormal range.  `within(got, ref, e, u)` is the condition  |got - ref| <= u (|ref| + e) + e + 2^-24  of the 16-bit BatchNorm
tests: e is the error of the value BEFORE its one rounding to the result's format.

Stage A, z.   zr = x64 w64^T, A = |x| |w|^T, e = (cin + 2) 2^-24 A (cin exact products added in fp32 in any order), one rounding to T.
Stage B, the BatchNorm part, evaluated ON THE OP'S OWN z (the GPU test reads it from the saved tensors; the CPU test uses the host
              emulation's): mean, invstd, y, running statistics, dgamma, dbeta against oracle/bn_oracle.py on that z with the bounds of
              the 16-bit BatchNorm op (bn_half_cases.fwd_error / bwd_error).
Stage C, gradients.  du64 from the oracle; the staged du is within d = u (|du64| + e_du) + e_du (+ 2^-24 in float16) of it, e_du from
              bwd_error.  dx64 = du64 w64: the staging error reaches it through |w|, the fp32 chain of cout exact products adds
              (cout + 2) 2^-24 of the absolute product:  E_dx = d |w| + (cout + 2) 2^-24 (|du64| + d) |w|.   dw64 = du64^T x64: chains of
              at most 128 rows in fp32, the chains summed in fp64:  E_dw = d^T |x| + ((128 + 2) 2^-24 + n 2^-53) (|du64| + d)^T |x|.
              One final rounding in the result's format (T, or fp32 for a master weight) closes each bound.

ReLU kink.  A pre-activation within the forward's evaluation error of zero may be masked either way, so for the gradient comparisons dy
is zeroed where |pre64| <= 4 (e + 2^-24); `stage_b` counts those elements and the tests require at most 1e-4 of them.
Construction.  x standard normal; w normal / sqrt(cin); gamma in [0.5, 1.5]; beta in [-0.5, 0.5]; dy standard normal.  |z| stays below 8
(the tests assert it), so float16 cannot overflow.
`emulate` evaluates the contract on the host - fp32 matmul of the widened operands, round_to, fp32 expressions - so that the CPU test can
show every reference inside every bound without a GPU."""
import functools

import numpy as np
import torch

from bn_half_cases import EPS24, UNIT, bwd_error, fwd_error, round64_to
from half_cases import round_to
from oracle import bn_oracle

SPLIT_SHAPE = (300, 64, 128)   # at least 3 weight-gradient splits, the last one ragged (asserted through fv2p_linear_bn_h_splits)
# (n, cin, cout), the smallest at which each path can go wrong: element-wise tails; around one wave and one 32-wide K step; multiples
# of 8 that are no multiples of 16 / 32; the decoder's channel pairs with ragged rows; the splits; the limits
SHAPES = [(2, 1, 1), (3, 5, 7), (130, 6, 20), (63, 16, 16), (64, 32, 16), (65, 33, 33), (129, 40, 72), (257, 160, 192), (515, 192, 160),
          SPLIT_SHAPE, (70, 1024, 512)]
MASTER_SHAPES = [(65, 33, 33), (257, 160, 192)]
EVAL_SHAPES = [(1, 5, 7), (65, 33, 33), (515, 192, 160)]
BITS_SHAPES = [SPLIT_SHAPE, (257, 160, 192)]
KINK_FRACTION = 1e-4
Z_MAX = 8.0
CHAIN = 128    # rows per fp32 accumulator chain of the weight gradient
EPS = 2.0 ** -10   # the modules' eps: about the decoder's 1e-3, and the same number as a float (the kernel's argument) and as a double


def _seed(n, cin, cout, dtype, tag):
    return (n * 1009 + cin * 131 + cout * 17 + (1 if dtype == torch.float16 else 2) * 5 + tag * 100003) % (2 ** 31)


@functools.lru_cache(maxsize=None)
def operands(n, cin, cout, dtype, wdtype, pdtype, affine=True, tag=0):
    """float64 arrays holding values of the case's formats: x, dy in `dtype`; w in `wdtype` (the module's weight) and wt = w rounded to
    `dtype` (what the op multiplies: the same array when wdtype is dtype); gamma, beta in `pdtype` (ones / zeros without affine)."""
    rng = np.random.default_rng(_seed(n, cin, cout, dtype, tag))
    x = round_to(rng.standard_normal((n, cin)), dtype)
    w = round_to(rng.standard_normal((cout, cin)) / np.sqrt(cin), wdtype)
    wt = round_to(w, dtype)
    gamma, beta = round_to(rng.uniform(0.5, 1.5, size=cout), pdtype), round_to(rng.uniform(-0.5, 0.5, size=cout), pdtype)
    if not affine:
        gamma, beta = np.ones(cout), np.zeros(cout)
    dy = round_to(rng.standard_normal((n, cout)), dtype)
    rm, rv = round_to(0.5 * rng.standard_normal(cout), pdtype), round_to(rng.uniform(0.5, 1.5, size=cout), pdtype)
    return dict(n=n, cin=cin, cout=cout, x=x, w=w, wt=wt, gamma=gamma, beta=beta, dy=dy, rm=rm, rv=rv)


def within(got, ref, e, u):
    """-> the element-wise ratio |got - ref| / (u (|ref| + e) + e + 2^-24): at most 1 inside the bound."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got - ref) / (u * (np.abs(ref) + e) + e + EPS24)


def stage_a(x, wt):
    """-> (zr, e): the float64 product and the fp32 accumulation error of its cin exact terms."""
    zr = x @ wt.T
    e = (x.shape[1] + 2) * EPS24 * (np.abs(x) @ np.abs(wt).T)
    return zr, e


def stage_b(z, gamma, beta, relu, dy, batch_stats=True, rm=None, rv=None, eps=EPS):
    """The BatchNorm part in float64 on the 16-bit pre-activation z (float64 array of T values) and its error terms.  batch_stats: the
    statistics of z; otherwise the running statistics rm / rv (eval mode).  dy comes back with the kink elements zeroed."""
    n = z.shape[0]
    if batch_stats:
        pre, (mean, invstd, xhat), _, _, _ = bn_oracle.bn_relu_forward(z, gamma, beta, None, None, 0, True, None, eps, False)
    else:
        pre, (mean, invstd, xhat), _, _, _ = bn_oracle.bn_relu_forward(z, gamma, beta, rm, rv, 0, False, None, eps, False)
    e, exh = fwd_error(z, mean, invstd, gamma, beta, None)
    kink = (np.abs(pre) <= 4 * (e + EPS24)) if relu else np.zeros(pre.shape, bool)
    dy = np.where(kink, 0.0, dy)
    y = np.maximum(pre, 0.0) if relu else pre
    du, dgamma, dbeta = bn_oracle.bn_relu_backward(dy, y, (mean, invstd, xhat), gamma, relu, batch_stats)
    dz = dy * ((y > 0) if relu else 1.0)
    e_du, e_dgamma = bwd_error(dz, xhat, exh, invstd, gamma, dz.mean(0), (dz * xhat).mean(0), batch_stats)
    # the statistics: fp64 sums of n values (n 2^-53 of the absolute sum), then ONE rounding to fp32 (two allowed, as the BatchNorm tests)
    m2 = (z * z).mean(0)
    e_mean = 2 * EPS24 * np.abs(mean) + n * 2.0 ** -53 * np.abs(z).mean(0)
    e_var = (n + 4) * 2.0 ** -53 * (m2 + mean * mean)
    e_invstd = 2 * EPS24 * invstd + 0.5 * invstd ** 3 * e_var
    return dict(pre=pre, y=y, mean=mean, invstd=invstd, xhat=xhat, e=e, kink=int(kink.sum()), dy=dy, dz=dz, du=du, dgamma=dgamma, dbeta=dbeta,
                e_du=e_du, e_dgamma=e_dgamma, e_mean=e_mean, e_invstd=e_invstd)


def running_step(z, rm, rv, nbt, momentum, pdtype, eps=EPS):
    """One training step of the running statistics on z from (rm, rv, nbt) in float64, rounded ONCE to the parameters' format (as
    bn_half_cases.exact_running does after every step).  -> (rm, rv, nbt, e_rm, e_rv): the float64 values before the rounding are the
    references; e_*: the fp64 evaluation error of the update ((n + 16) 2^-53 of its absolute terms)."""
    n = z.shape[0]
    m = None if momentum is None else float(np.float32(momentum))   # the momentum the kernel is handed: a float
    _, (mean, _, _), rm2, rv2, nbt2 = bn_oracle.bn_relu_forward(z, 1.0, 0.0, rm, rv, nbt, True, m, eps, False)
    scale = (n + 16) * 2.0 ** -53
    e_rm = scale * (np.abs(rm) + np.abs(z).mean(0))
    e_rv = scale * (np.abs(rv) + 2.0 * (z * z).mean(0) * n / max(n - 1, 1))
    return rm2, rv2, nbt2, e_rm, e_rv


def stage_c(du, e_du, x, wt, dtype):
    """-> (dx, E_dx, dw, E_dw) from the oracle's du64 and its staging error."""
    u = UNIT[dtype]
    n, cout = du.shape
    d = u * (np.abs(du) + e_du) + e_du + (EPS24 if dtype == torch.float16 else 0.0)
    staged = np.abs(du) + d
    dx = du @ wt
    e_dx = d @ np.abs(wt) + (cout + 2) * EPS24 * (staged @ np.abs(wt))
    dw = du.T @ x
    e_dw = d.T @ np.abs(x) + ((CHAIN + 2) * EPS24 + n * 2.0 ** -53) * (staged.T @ np.abs(x))
    return dx, e_dx, dw, e_dw


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def emulate(ops, dtype, pdtype, wdtype, relu, batch_stats=True, eps=EPS):
    """The contract on the host: fp32 matmul of the widened operands, round_to, the kernels' fp32 expressions, fp64 sums.  -> float64
    arrays holding the values the op would store (z, y, du, dx in T; dw in the weight's format; dgamma / dbeta in the parameters'; mean /
    invstd fp32).  dy: the case's, masked by `stage_b` on the emulated z (the caller passes the masked dy in)."""
    x, wt = _f32(ops["x"]), _f32(ops["wt"])
    n = x.shape[0]
    z = round_to((x @ wt.T).astype(np.float64), dtype)
    z32 = _f32(z)
    if batch_stats:
        mean64, var64 = z.mean(0), np.maximum((z * z).mean(0) - z.mean(0) ** 2, 0.0)
        mean, invstd = _f32(mean64), _f32(1.0 / np.sqrt(var64 + np.float64(np.float32(eps))))
    else:
        mean, invstd = _f32(ops["rm"]), _f32(1.0 / np.sqrt(ops["rv"] + eps))
    ga, be = _f32(ops["gamma"]), _f32(ops["beta"])
    xhat = (z32 - mean) * invstd
    t = xhat * ga + be
    y = round_to(np.where(relu & (t <= 0), np.float32(0), t).astype(np.float64), dtype)

    def backward(dy):
        dz = np.where(relu & ~(t > 0), np.float32(0), _f32(dy))
        s1, s2 = dz.astype(np.float64).sum(0), (dz.astype(np.float64) * xhat.astype(np.float64)).sum(0)
        c1, c2 = (_f32(s1 / n), _f32(s2 / n)) if batch_stats else (np.zeros_like(mean), np.zeros_like(mean))
        du = round_to(((ga * invstd) * ((dz - c1) - xhat * c2)).astype(np.float64), dtype)
        du32 = _f32(du)
        dx = round_to((du32 @ wt).astype(np.float64), dtype)
        dw64 = np.zeros((wt.shape[0], wt.shape[1]))
        for r0 in range(0, n, CHAIN):   # fp32 chains of at most 128 rows, summed in fp64
            dw64 += (du32[r0:r0 + CHAIN].T @ x[r0:r0 + CHAIN]).astype(np.float64)
        dw = round64_to(dw64, wdtype)
        return dict(du=du, dx=dx, dw=dw, dgamma=round64_to(s2, pdtype), dbeta=round64_to(s1, pdtype))

    return dict(z=z, y=y, mean=mean.astype(np.float64), invstd=invstd.astype(np.float64)), backward
