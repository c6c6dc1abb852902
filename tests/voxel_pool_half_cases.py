"""Shared builders of the 16-bit voxel-pool tests (test_voxel_pool_half_cpu.py / test_voxel_pool_half_gpu.py): the cases and the
restatement of voxel_pool_cases, with F and grad_out rounded to float16 / bfloat16 first (kept as float32 values on the host, so that
the float64 truth, the float32 yardstick and the GPU op all start from the same numbers).

Bound of the 16-bit tensors (out, grad_F), element-wise, the rule of the other 16-bit tests:
    |got - ref64| <= u (|ref64| + e) + e + 2^-24,    u = 2^-11 (float16) / 2^-8 (bfloat16): the one rounding at the store,
    e = K max|host32 - ref64| over the tensor: what a float32 evaluation of the same formula is allowed to be away from float64
    (K of f64_calibration), 2^-24 for a result that is exactly zero in one of the two."""
import functools

import numpy as np
import torch

import voxel_pool_cases as vc
from f64_calibration import K

DTYPES = [torch.float16, torch.bfloat16]
UNIT = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
EPS24 = 2.0 ** -24


def rounded(d, dtype):
    """The case with F and grad_out rounded to `dtype` (as float32 values); everything else is shared with `d`."""
    d = dict(d)
    d["f"] = d["f"].to(dtype).float()
    d["grad_out"] = d["grad_out"].to(dtype).float()
    return d


def build(case, dtype, seed=0):
    return rounded(vc.build(case, seed), dtype)


def references(d, momentum, training, steps):
    """(gradient mask, float64 steps, float32 steps) of the restatement on the inputs `d`, the cap on masked cells asserted as
    voxel_pool_cases.reference asserts it."""
    _, marg = vc.restated(d, momentum, training, torch.float64, 1)
    mask = (marg >= vc.MARGIN).to(torch.float32)
    assert float((mask == 0).float().mean()) <= vc.MAX_MASKED, "too many cells within MARGIN of a tie: choose another seed"
    r64, _ = vc.restated(d, momentum, training, torch.float64, steps, mask)
    r32, _ = vc.restated(d, momentum, training, torch.float32, steps, mask)
    return mask, r64, r32


@functools.lru_cache(maxsize=None)
def reference(name, dtype, momentum, training, steps=1):
    """(inputs, gradient mask, float64 steps, float32 steps) of a named case: computed once, shared, never modified."""
    d = build(vc.CASES[name], dtype)
    return (d,) + references(d, momentum, training, steps)


def within16(what, got, host32, ref64, dtype, report=print):
    """The element-wise bound above; prints the largest ratio before it judges."""
    got, host32, ref64 = (t.detach().cpu().double().numpy() for t in (got, host32, ref64))
    e = K * float(np.abs(host32 - ref64).max()) if ref64.size else 0.0
    bound = UNIT[dtype] * (np.abs(ref64) + e) + e + EPS24
    ratio = np.abs(got - ref64) / bound
    worst = float(ratio.max()) if ratio.size else 0.0
    report(f"  {what:28s} max |err| / bound = {worst:.3f}  (e {e:.2e}, max |ref| {float(np.abs(ref64).max()) if ref64.size else 0.0:.2e})")
    assert np.isfinite(got).all() and worst <= 1.0, f"{what}: {worst:.3f} of the bound"
