"""Cases of the 16-bit fused grid set-abstraction (csrc/sa_fused.hip) with their float64 references.  Host only; not a test module.

Random cases: the generators, shapes, padded tails and single-neighbour centres of tests/test_pointnet2_gpu.py's fused cases, the
operands cast to float16 / bfloat16.  The reference is the kernel's stated arithmetic in float64:
    h1r = (P.float() - Q.float()).relu().to(dtype).double()      W2r = W2.to(dtype).double()
    a = einsum(W2r, h1r)      A = einsum(|W2r|, |h1r|)      out = max(0, max_s a)
Every bound below is derived from the number formats (u = 2^-11 / 2^-8, fp32 accumulation 2^-24 per addition); nothing is measured.
DH1_STAGED_16BIT mirrors the kernel file's header: the dh1 rows behind grad_point are staged in 16 bits (u_s = u)."""
import functools

import torch

UNIT = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
DTYPES = [torch.float16, torch.bfloat16]
F32 = 2.0 ** -24
DH1_STAGED_16BIT = True

# (r, n, m, s): tests/test_pointnet2_gpu.py's four, one above the fp32 backward's n <= 884, and one above the 8192 samples per RoI up to which
# grad_point is summed inside one workgroup (beyond: scatter_add_h)
SHAPES = [(5, 100, 30, 16), (3, 512, 216, 32), (2, 640, 17, 16), (1, 64, 1, 32), (2, 1000, 17, 16), (1, 64, 300, 32)]


def shape_id(shape):
    return "r%d-n%d-m%d-s%d" % shape


def dtype_id(dt):
    return str(dt).split(".")[-1]


@functools.lru_cache(maxsize=None)
def inputs(shape):
    """fp32 host tensors: per_point, per_centre, w2, idx (int32), grad_out - tests/test_pointnet2_gpu.py:241-251's draws, in its order."""
    r, n, m, s = shape
    g = torch.Generator().manual_seed(r * 1000 + n)
    pp = torch.randn(r, n, 64, generator=g)
    pc = torch.randn(r, m, 64, generator=g) * 0.5
    w2 = torch.randn(64, 64, generator=g) * 0.2
    idx = torch.randint(0, n, (r, m, s), generator=g, dtype=torch.int32)
    idx[:, :, s // 2:] = idx[:, :, :1]                       # padded tail: repeats of the first hit
    idx[:, ::3, :] = idx[:, ::3, :1]                         # centres with a single distinct neighbour
    go = torch.randn(r, m, 64, generator=g)
    return pp, pc, w2, idx, go


def gather_rows(p, idx):
    """p (r, n, c), idx (r, m, s) -> (r, m, s, c); an index outside [0, n) reads as a row of zeros."""
    r, n, c = p.shape
    ok = (idx >= 0) & (idx < n)
    flat = idx.long().clamp(0, n - 1).reshape(r, -1)
    rows = torch.gather(p, 1, flat.unsqueeze(-1).expand(-1, -1, c)).reshape(*idx.shape, c)
    return rows * ok.unsqueeze(-1).to(p.dtype)


def forward_ref(pp, pc, w2, idx, dt):
    """The stated arithmetic in float64 on host tensors already cast to dt (w2 in dt or fp32).  -> dict(h1, w, a, A, out, e)."""
    h1 = (gather_rows(pp.float(), idx) - pc.float().unsqueeze(2)).relu().to(dt).double()       # (r, m, s, 64)
    w = w2.to(dt).double()
    a = torch.einsum("oc,rmsc->rmso", w, h1)
    A = torch.einsum("oc,rmsc->rmso", w.abs(), h1.abs())
    e = 66 * F32 * A.amax(dim=2)          # 64 exact products summed in fp32 in any order
    return dict(h1=h1, w=w, a=a, A=A, out=a.amax(dim=2).clamp_min(0.0), e=e)


@functools.lru_cache(maxsize=None)
def case(shape, dt):
    """-> dict: the 16-bit host operands (pp, pc, go in dt; w2 fp32, and w2.to(dt)), idx, and forward_ref's results."""
    pp, pc, w2, idx, go = inputs(shape)
    c = dict(pp=pp.to(dt), pc=pc.to(dt), w2=w2, w2h=w2.to(dt), idx=idx, go=go.to(dt), shape=shape, dt=dt)
    c.update(forward_ref(c["pp"], c["pc"], w2, idx, dt))
    return c


def forward_bound(c):
    """|got - ref| <= u (|ref| + e) + e + 2^-24: e for the fp32 accumulation (the maximum moves by at most the largest e of its samples),
    u (|ref| + e) for the one rounding of the result, 2^-24 for float16 results in the subnormal range."""
    u = UNIT[c["dt"]]
    return u * (c["out"].abs() + c["e"]) + c["e"] + F32


def first_true(mask, dim):
    """Index of the first True along dim (the size of dim where there is none)."""
    return (mask.long().cumsum(dim) == 0).sum(dim)


def arg_sets(c):
    """The reference's view of arg per (centre, channel): `want` (the earliest slot holding the winning point, or 255) where the decision
    is beyond rounding - the best value exceeds by more than 2 e both zero and the best value held by a different point, or lies more
    than 2 e below zero - and `strict` marking those pairs.  Everything else is a near-tie."""
    a, idx, e = c["a"], c["idx"].long(), c["e"]
    s = a.shape[2]
    v1 = a.amax(dim=2)                                                        # (r, m, 64)
    slot = first_true(a == v1.unsqueeze(2), 2)                                # some slot holding the maximum
    pt = torch.gather(idx, 2, slot.clamp(max=s - 1).reshape(*idx.shape[:2], -1)).reshape(v1.shape)   # (r, m, 64): the winning point
    same = idx.unsqueeze(-1) == pt.unsqueeze(2)                               # (r, m, s, 64)
    other = a.masked_fill(same, float("-inf")).amax(dim=2)
    first = first_true(same, 2)
    live = (v1 > 2 * e) & (v1 - other > 2 * e)
    dead = v1 < -2 * e
    want = torch.where(live, first, torch.full_like(first, 255))
    return dict(want=want, strict=live | dead, v1=v1)


def backward_ref(c, arg, w32):
    """float64 gradients routed by `arg` (r, m, 64; long, 255 = none) with their bounds.  -> dict(name: (ref, bound))."""
    dt, idx = c["dt"], c["idx"]
    r, n, m, s = c["shape"]
    u = UNIT[dt]
    us = u if DH1_STAGED_16BIT else 0.0
    h1, w = c["h1"], c["w"]
    hit = arg.unsqueeze(2) == torch.arange(s).view(1, 1, s, 1)               # (r, m, s, 64)
    dh2 = c["go"].double().unsqueeze(2) * hit
    dh1 = torch.einsum("oc,rmso->rmsc", w, dh2) * (h1 > 0)
    B = torch.einsum("oc,rmso->rmsc", w.abs(), dh2.abs())
    tail = lambda ref, e, unit: unit * (ref.abs() + e) + e + F32
    res = {}
    res["grad_centre"] = (-dh1.sum(2), tail(-dh1.sum(2), (us + (66 + s) * F32) * B.sum(2), u))
    ok = ((idx >= 0) & (idx < n)).reshape(r, -1)
    flat = idx.long().clamp(0, n - 1).reshape(r, -1)
    gp, gb, cnt = torch.zeros(r, n, 64, dtype=torch.float64), torch.zeros(r, n, 64, dtype=torch.float64), torch.zeros(r, n, dtype=torch.float64)
    for k in range(r):
        gp[k].index_add_(0, flat[k], dh1[k].reshape(-1, 64) * ok[k].unsqueeze(-1))
        gb[k].index_add_(0, flat[k], B[k].reshape(-1, 64) * ok[k].unsqueeze(-1))
        cnt[k].index_add_(0, flat[k], ok[k].double())
    res["grad_point"] = (gp, tail(gp, (us + (66 + cnt.unsqueeze(-1)) * F32) * gb, u))
    gw = torch.einsum("rmso,rmsc->oc", dh2, h1)
    ew = r * m * s * F32 * torch.einsum("rmso,rmsc->oc", dh2.abs(), h1.abs())
    res["grad_w2"] = (gw, tail(gw, ew, 0.0 if w32 else u))
    return res


@functools.lru_cache(maxsize=None)
def exact_case(s):
    """P, Q integers in [-8, 8], W2 in {-1, 0, 1}, grad_out integers in [-2, 2], shape (2, 64, 17, s): every product and every sum is
    exact in fp32 (|a| <= 1024, |dh1| <= 128), so every result equals the float64 reference .to(dtype) bit for bit in both formats."""
    r, n, m = 2, 64, 17
    g = torch.Generator().manual_seed(41 + s)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float()
    pp, pc, w2, go = ri(-8, 8, r, n, 64), ri(-8, 8, r, m, 64), ri(-1, 1, 64, 64), ri(-2, 2, r, m, 64)
    idx = torch.randint(0, n, (r, m, s), generator=g, dtype=torch.int32)
    idx[:, :, s // 2:] = idx[:, :, :1]
    idx[:, ::3, :] = idx[:, ::3, :1]
    c = dict(pp=pp, pc=pc, w2=w2, idx=idx, go=go, shape=(r, n, m, s), dt=torch.float64)
    h1 = (gather_rows(pp.double(), idx) - pc.double().unsqueeze(2)).relu()
    a = torch.einsum("oc,rmsc->rmso", w2.double(), h1)
    v1 = a.amax(dim=2)
    arg = torch.where(v1 > 0, first_true(a == v1.unsqueeze(2), 2), torch.full(v1.shape, 255, dtype=torch.long))   # the first arg-max in sample order
    c.update(h1=h1, w=w2.double(), a=a, out=v1.clamp_min(0.0), arg=arg)
    grads = backward_ref(dict(c, dt=torch.float16), arg, True)     # the bounds are not used: only the float64 values
    c.update({k: v[0] for k, v in grads.items()})
    assert float(a.abs().max()) <= 1024 and float(c["grad_w2"].abs().max()) < 2 ** 24 and float(c["grad_point"].abs().max()) < 2 ** 24
    return c
