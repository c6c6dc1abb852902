"""Voxel pooling on float16 / bfloat16 rows under torch.autocast (the Fmt16 instances of csrc/voxel_pool.hip through
voxel_pool_fused / NeighborVoxelSAModuleMSG).  Two yardsticks: the fp32 op on the same (rounded) numbers, which the 16-bit op must
reproduce bit for bit up to the one rounding of its 16-bit outputs; and, independent of that sibling, the float64 restatement of
voxel_pool_cases on the CPU with the element-wise bound of voxel_pool_half_cases."""
import contextlib
import copy

import pytest
import torch

import voxel_pool_cases as vc
import voxel_pool_half_cases as hc
from f64_calibration import FLOOR, K, rel_l2
from pcdet.ops.pointnet2.pointnet2_stack import voxel_pool_fused, voxel_pool_modules

pytestmark = pytest.mark.gpu

F32_OUTPUTS = ["grad_w", "grad_gamma", "grad_beta", "running_mean", "running_var"]
OTHER = {torch.float16: torch.bfloat16, torch.bfloat16: torch.float16}


def _steps(d, gpu, momentum, training, steps, dtype, mask=None, grads=(True, True)):
    """`steps` forward + backward passes of the fused op on the case `d` -> per-step dicts like voxel_pool_cases.restated.
    dtype float32: the fp32 op outside autocast; float16 / bfloat16: rows and grad_out of that dtype inside torch.autocast."""
    conv, bn = vc.modules(d, momentum, training, device=gpu)
    f = d["f"].to(gpu).to(dtype).requires_grad_(grads[0])
    xyz, new_xyz, idx, empty = (d[k].to(gpu) for k in ("xyz", "new_xyz", "idx", "empty"))
    for p in (conv.weight, bn.weight, bn.bias):
        p.requires_grad_(grads[1])
    go = (d["grad_out"] * (1 if mask is None else mask)).to(gpu).to(dtype)
    res = []
    with (contextlib.nullcontext() if dtype == torch.float32 else torch.autocast("cuda", dtype=dtype)):
        for _ in range(steps):
            for t in (f, conv.weight, bn.weight, bn.bias):
                t.grad = None
            assert voxel_pool_fused.supported(f, idx, conv, bn, xyz, new_xyz)
            out = voxel_pool_fused.voxel_pool_max(f, xyz, new_xyz, idx, empty, conv, bn)
            assert out is not None and out.shape == d["grad_out"].shape and out.dtype == dtype
            out.backward(go)
            res.append(dict(out=out.detach().clone(), grad_f=f.grad, grad_w=conv.weight.grad, grad_gamma=bn.weight.grad, grad_beta=bn.bias.grad,
                            running_mean=bn.running_mean.clone(), running_var=bn.running_var.clone(),
                            num_batches_tracked=int(bn.num_batches_tracked)))
    torch.cuda.synchronize()
    return res


def _same_arithmetic(h, f, dtype, what):
    """The 16-bit op's outputs against the fp32 op's on the same numbers: no tolerance."""
    assert h["out"].dtype == dtype and h["grad_f"].dtype == dtype
    assert torch.equal(h["out"], f["out"].to(dtype)), f"{what}: out"
    for k in F32_OUTPUTS:
        assert h[k].dtype == torch.float32 and torch.equal(h[k], f[k]), f"{what}: {k}"
    assert h["num_batches_tracked"] == f["num_batches_tracked"], what
    assert torch.equal(h["grad_f"], f["grad_f"].to(dtype)), f"{what}: grad_f"


# ---- 1. the same arithmetic as the fp32 op ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", hc.DTYPES)
@pytest.mark.parametrize("mode", [0.1, None, "eval"])
@pytest.mark.parametrize("name", list(vc.CASES))
def test_same_arithmetic_as_fp32_op(gpu, name, mode, dtype):
    d = hc.build(vc.CASES[name], dtype)
    training, momentum, steps = (False, 0.1, 1) if mode == "eval" else (True, mode, 2)
    half = _steps(d, gpu, momentum, training, steps, dtype)
    full = _steps(d, gpu, momentum, training, steps, torch.float32)
    for step in range(steps):
        _same_arithmetic(half[step], full[step], dtype, f"{name} {mode} step {step + 1}")
        assert half[step]["num_batches_tracked"] == (step + 1 if training else 0)


# ---- 2. against float64, independent of the sibling -------------------------------------------------------------------------------
def _against_f64(hip, r32, r64, dtype, training):
    for k in F32_OUTPUTS[:3] + (F32_OUTPUTS[3:] if training else []):
        vc.within(k, hip[k], r32[k], r64[k])
    for k in ("out", "grad_f"):
        assert hip[k].dtype == dtype
        hc.within16(k, hip[k], r32[k], r64[k], dtype)


@pytest.mark.parametrize("dtype", hc.DTYPES)
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("name", ["c12", "config", "blocks", "two_samples"])
def test_against_float64(gpu, name, training, dtype):
    d, mask, r64, r32 = hc.reference(name, dtype, 0.1, training)
    hip = _steps(d, gpu, 0.1, training, 1, dtype, mask)[0]
    print(f"{name} {dtype} training={training}")
    _against_f64(hip, r32[0], r64[0], dtype, training)
    if not training:
        assert torch.equal(hip["running_mean"].cpu(), d["running_mean"]) and torch.equal(hip["running_var"].cpu(), d["running_var"])
        assert hip["num_batches_tracked"] == 0


# ---- 3. edges ----------------------------------------------------------------------------------------------------------------------
def _tie_case(dtype):
    """4 queries of 4 samples over 10 rows, 8 channels (the case of test_voxel_pool_gpu, F and grad_out rounded).  Query 0 meets rows 5
    and 2, which are identical and dominate (sample 1 before sample 2); query 1 is one hit padded three times; query 2 meets row 8,
    which the NaN test fills; query 3 is empty."""
    d = vc.build(((4,), (10,), 4, 8, 0.0))
    d["f"][5] = 10.0
    d["f"][2] = d["f"][5]
    d["xyz"][2] = d["xyz"][5]
    d["f"][3] = 10.0
    d["idx"] = torch.tensor([[7, 5, 2, 7], [3, 3, 3, 3], [8, 9, 8, 8], [0, 0, 0, 0]], dtype=torch.int32)
    d["empty"] = torch.tensor([False, False, False, True])
    d["gamma"] = d["gamma"] * 0.1   # the position branch stays far below the dominating rows
    return hc.rounded(d, dtype)


@pytest.mark.parametrize("dtype", hc.DTYPES)
def test_ties(gpu, dtype):
    d = _tie_case(dtype)
    hip = _steps(d, gpu, 0.1, True, 1, dtype)[0]
    out, gf, go = hip["out"].cpu(), hip["grad_f"].cpu(), d["grad_out"].to(dtype)
    zero = torch.zeros(8, dtype=dtype)
    assert bool((out[:2].float() > 5).all())
    assert torch.equal(gf[5], go[0]) and torch.equal(gf[2], zero), "a tie goes to the lower sample number"
    assert torch.equal(gf[7], zero)
    assert torch.equal(gf[3], go[1]), "a padded list's gradient lands once"
    assert torch.equal(gf[0], zero), "an empty query sends no gradient to row 0"


@pytest.mark.parametrize("dtype", hc.DTYPES)
def test_nan_cells(gpu, dtype):
    d = _tie_case(dtype)
    d["f"][8, 1] = float("nan")
    d["f"][9, 6] = float("nan")
    with torch.no_grad():
        conv, bn = vc.modules(d, 0.1, True, device=gpu)
        args = [d[k].to(gpu) for k in ("xyz", "new_xyz", "idx", "empty")]
        with torch.autocast("cuda", dtype=dtype):
            out = voxel_pool_fused.voxel_pool_max(d["f"].to(gpu).to(dtype), *args, conv, bn)
        conv32, bn32 = vc.modules(d, 0.1, True, device=gpu)
        want = voxel_pool_fused.voxel_pool_max(d["f"].to(gpu), *args, conv32, bn32)
    assert out is not None and out.dtype == dtype and want is not None and want.dtype == torch.float32
    assert torch.equal(torch.isnan(out), torch.isnan(want))
    assert torch.isnan(out).sum() == 2 and bool(torch.isnan(out[2, 1])) and bool(torch.isnan(out[2, 6]))
    keep = ~torch.isnan(want)
    assert torch.equal(out[keep], want.to(dtype)[keep])


@pytest.mark.parametrize("dtype", hc.DTYPES)
def test_out_of_range_indices(gpu, dtype):
    """Entries N + 5 and -3 behave as rows of zeros and receive no gradient; every kernel checks a row against [0, N) before it reads."""
    ms, ns, s, c, _ = case = ((40,), (30,), 8, 16, 0.2)
    d = hc.build(case, dtype)
    d["idx"] = d["idx"].clone()
    live = (~d["empty"]).nonzero().flatten()
    d["idx"][live[0], 1] = ns[0] + 5
    d["idx"][live[1], 0] = -3
    d["idx"][live[2], s - 1] = -3
    mask, r64, r32 = hc.references(d, 0.1, True, 1)
    hip = _steps(d, gpu, 0.1, True, 1, dtype, mask)[0]
    assert hip["grad_f"].shape == (ns[0], c) and bool(torch.isfinite(hip["grad_f"]).all())
    _against_f64(hip, r32[0], r64[0], dtype, True)


# ---- 4. run to run -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", hc.DTYPES)
def test_run_to_run(gpu, dtype):
    d = hc.build(vc.CASES["two_samples"], dtype)
    a, b = _steps(d, gpu, 0.1, True, 1, dtype)[0], _steps(d, gpu, 0.1, True, 1, dtype)[0]
    for k in ["out", "grad_f"] + F32_OUTPUTS:
        assert torch.equal(a[k], b[k]), k


# ---- 5. routing --------------------------------------------------------------------------------------------------------------------
def _state(bn):
    return {k: v.clone() for k, v in bn.state_dict().items()}


def _declines(f, d, gpu, conv, bn):
    args = [d[k].to(gpu) for k in ("xyz", "new_xyz", "idx", "empty")]
    before = _state(bn)
    assert voxel_pool_fused.supported(f, args[2], conv, bn, args[0], args[1]) is False
    assert voxel_pool_fused.voxel_pool_max(f, *args, conv, bn) is None
    after = _state(bn)
    assert all(torch.equal(before[k], after[k]) for k in before)


@pytest.mark.parametrize("dtype", hc.DTYPES)
def test_routing(gpu, dtype):
    d = hc.build(vc.CASES["c12"], dtype)
    conv, bn = vc.modules(d, 0.1, True, device=gpu)
    f16, f32 = d["f"].to(gpu).to(dtype), d["f"].to(gpu)
    taken = _steps(d, gpu, 0.1, True, 1, dtype)[0]                       # asserts supported() and the result's dtype under autocast
    assert taken["out"].dtype == dtype and taken["grad_f"].dtype == dtype
    _declines(f16, d, gpu, conv, bn)                                    # 16-bit rows outside autocast
    with torch.autocast("cuda", dtype=OTHER[dtype]):
        _declines(f16, d, gpu, conv, bn)                                # ... under an autocast of the other 16-bit dtype
    with torch.autocast("cuda", dtype=dtype):
        _declines(f32, d, gpu, conv, bn)                                # float32 rows under autocast
        _declines(f32.double(), d, gpu, conv, bn)                       # float64 rows
        conv_h, bn_h = vc.modules(d, 0.1, True, dtype=dtype, device=gpu)
        _declines(f16, d, gpu, conv_h, bn_h)                            # 16-bit parameters
        _declines(f16, d, gpu, conv_h, bn)
        _declines(f16, d, gpu, conv, bn_h)
    _declines(f32.double(), d, gpu, conv, bn)
    _declines(f16, d, gpu, conv_h, bn_h)


@pytest.mark.parametrize("dtype", hc.DTYPES)
def test_grad_out_of_another_dtype(gpu, dtype):
    """Nothing is cast on the way to the library: a gradient that does not have the rows' dtype is an error.  (autograd itself casts
    the gradient handed to Tensor.backward to the output's dtype, so the op's backward is called directly.)"""
    d = hc.build(vc.CASES["c12"], dtype)
    conv, bn = vc.modules(d, 0.1, True, device=gpu)
    f = d["f"].to(gpu).to(dtype).requires_grad_(True)
    with torch.autocast("cuda", dtype=dtype):
        out = voxel_pool_fused.voxel_pool_max(f, *(d[k].to(gpu) for k in ("xyz", "new_xyz", "idx", "empty")), conv, bn)
    saved = out.grad_fn.saved
    for wrong in (torch.float32, OTHER[dtype]):
        with pytest.raises(TypeError):
            voxel_pool_fused._bwd(saved, d["grad_out"].to(gpu).to(wrong))
    grads = voxel_pool_fused._bwd(saved, d["grad_out"].to(gpu).to(dtype))
    assert grads[0].dtype == dtype and grads[5].dtype == torch.float32


@pytest.mark.parametrize("dtype", hc.DTYPES)
def test_no_float32_image_of_the_rows(gpu, dtype, monkeypatch):
    """A forward + backward allocates no float32 tensor of M C or N C elements: out, g and grad_F stay in the rows' dtype.  Only
    the tensors of G.new are watched here; that the workspace holds no such region either rests on the size bound of
    test_voxel_pool_half_cpu.test_backward_workspace_query (the 16-bit workspace is 2 M C bytes below the fp32 one)."""
    ms, ns, s, c, _ = vc.CASES["config"]
    m, n = sum(ms), sum(ns)
    d = hc.build(vc.CASES["config"], dtype)
    made = []
    real = voxel_pool_fused.G.new

    def new(like, shape, dtype=torch.float32, fill=None):
        t = real(like, shape, dtype, fill)
        made.append((t.dtype, t.numel()))
        return t
    monkeypatch.setattr(voxel_pool_fused.G, "new", new)
    _steps(d, gpu, 0.1, True, 1, dtype)
    assert (dtype, m * c) in made and (dtype, n * c) in made and (torch.uint8, m * c) in made
    assert not [x for x in made if x[0] == torch.float32 and x[1] in (m * c, n * c)], made


# ---- 6. the module ----------------------------------------------------------------------------------------------------------------
def _module(gpu, cmid, seed=0):
    torch.manual_seed(seed)
    mod = voxel_pool_modules.NeighborVoxelSAModuleMSG(query_ranges=[[1, 2, 2], [1, 3, 3]], radii=[0.25, 0.4], nsamples=[16, 16],
                                                      mlps=[[8, cmid, 16], [8, cmid, 16]], pool_method="max_pool")
    with torch.no_grad():   # away from the constant initialisation of the BatchNorms
        for m in mod.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.3)
    return mod.to(gpu)


def _run_module(mod, occ, gpu, fused, dtype):
    mod = copy.deepcopy(mod)
    mod.FUSED = fused
    t = {k: v.to(gpu) for k, v in occ.items()}
    with torch.autocast("cuda", dtype=dtype):
        out = mod(t["xyz"], t["xyz_batch_cnt"], t["new_xyz"], t["new_xyz_batch_cnt"], t["new_coords"], t["features"], t["vol"])
    (out.float() * t["grad_out"]).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), {n: p.grad for n, p in mod.named_parameters()}


def _lists(mod, occ, gpu):
    t = {k: v.to(gpu) for k, v in occ.items()}
    coords = t["new_coords"][:, [0, 3, 2, 1]].contiguous()
    res = []
    for g in mod.groupers:
        idx, empty = g.query(coords, t["xyz"], t["xyz_batch_cnt"], t["new_xyz"], t["new_xyz_batch_cnt"], t["vol"])
        res.append((idx.cpu(), empty.cpu()))
    return res


@pytest.mark.parametrize("dtype", hc.DTYPES)
def test_module(gpu, dtype, monkeypatch):
    """The module under autocast, FUSED on against off (what the tree computed before the 16-bit op), both against the float64
    restatement.  Measured on one MI355X, rel_l2 to float64, fused / grouped: see DESIGN 3.5a."""
    occ = vc.occupancy((300, 220), (90, 70))
    mod = _module(gpu, 32)
    lists = _lists(mod, occ, gpu)
    assert all(0 < int(e.sum()) < e.numel() for _, e in lists), "the occupancy should leave some queries empty, not all"
    o64, g64, _, _ = vc.module_restated(mod, occ, lists, torch.float64)
    returned = []
    real = voxel_pool_fused.voxel_pool_max
    monkeypatch.setattr(voxel_pool_fused, "voxel_pool_max", lambda *a: returned.append(real(*a)) or returned[-1])
    runs = {}
    for fused in (True, False):
        returned.clear()
        runs[fused] = _run_module(mod, occ, gpu, fused, dtype)
        assert len(returned) == (2 if fused else 0)
        assert all(r is not None and r.dtype == dtype for r in returned)
    (out_f, grads_f), (out_u, grads_u) = runs[True], runs[False]
    assert out_f.dtype == out_u.dtype == dtype
    assert set(grads_f) == set(grads_u) == set(g64)
    print(f"module {dtype}: rel_l2 to float64, fused | grouped")
    rows = [("out", out_f, out_u, o64)] + [("grad " + n, grads_f[n], grads_u[n], g64[n]) for n in g64]
    bad = []
    for what, a, b, truth in rows:
        assert a.dtype == b.dtype, what
        d_f, d_u = rel_l2(a, truth), rel_l2(b, truth)
        bound = max(K * d_u, FLOOR)
        print(f"  {what:34s} fused {d_f:.2e}  grouped {d_u:.2e}  bound {bound:.2e}")
        if not d_f <= bound:
            bad.append(f"{what}: fused {d_f:.2e}, grouped {d_u:.2e}, bound {bound:.2e}")
    assert not bad, bad
