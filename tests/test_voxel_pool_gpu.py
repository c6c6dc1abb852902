"""Voxel pooling on the GPU (csrc/voxel_pool.hip through voxel_pool_fused / NeighborVoxelSAModuleMSG) against the grouped
restatement of voxel_pool_cases: float64 on the CPU is the truth, the same code in float32 the yardstick."""
import copy

import pytest
import torch

import voxel_pool_cases as vc
from pcdet.ops.pointnet2.pointnet2_stack import voxel_pool_fused, voxel_pool_modules

pytestmark = pytest.mark.gpu

FLOATS = ["out", "grad_f", "grad_w", "grad_gamma", "grad_beta", "running_mean", "running_var"]


def _dev(d, gpu, *names):
    return [d[k].to(gpu) for k in names]


def _hip_steps(d, gpu, momentum, training, steps, mask=None, grads=(True, True)):
    """`steps` forward + backward passes of the fused op -> per-step dicts like voxel_pool_cases.restated."""
    conv, bn = vc.modules(d, momentum, training, device=gpu)
    f, xyz, new_xyz, idx, empty = _dev(d, gpu, "f", "xyz", "new_xyz", "idx", "empty")
    f.requires_grad_(grads[0])
    for p in (conv.weight, bn.weight, bn.bias):
        p.requires_grad_(grads[1])
    go = d["grad_out"].to(gpu) * (1 if mask is None else mask.to(gpu))
    res = []
    for _ in range(steps):
        for t in (f, conv.weight, bn.weight, bn.bias):
            t.grad = None
        assert voxel_pool_fused.supported(f, idx, conv, bn, xyz, new_xyz)
        out = voxel_pool_fused.voxel_pool_max(f, xyz, new_xyz, idx, empty, conv, bn)
        assert out is not None and out.shape == d["grad_out"].shape
        out.backward(go)
        res.append(dict(out=out.detach().clone(), grad_f=f.grad, grad_w=conv.weight.grad, grad_gamma=bn.weight.grad, grad_beta=bn.bias.grad,
                        running_mean=bn.running_mean.clone(), running_var=bn.running_var.clone(),
                        num_batches_tracked=int(bn.num_batches_tracked)))
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("momentum", [0.1, None])
@pytest.mark.parametrize("name", list(vc.CASES))
def test_training(gpu, name, momentum):
    d, mask, r64, r32 = vc.reference(name, momentum, True)
    hip = _hip_steps(d, gpu, momentum, True, 2, mask)
    for step in range(2):
        print(f"{name} momentum={momentum} step {step + 1}")
        for k in FLOATS:
            vc.within(k, hip[step][k], r32[step][k], r64[step][k])
        assert hip[step]["num_batches_tracked"] == r64[step]["num_batches_tracked"] == step + 1


@pytest.mark.parametrize("name", list(vc.CASES))
def test_eval(gpu, name):
    d, mask, r64, r32 = vc.reference(name, 0.1, False, 1)
    hip = _hip_steps(d, gpu, 0.1, False, 1, mask)[0]
    for k in FLOATS[:5]:
        vc.within(k, hip[k], r32[0][k], r64[0][k])
    assert torch.equal(hip["running_mean"].cpu(), d["running_mean"]) and torch.equal(hip["running_var"].cpu(), d["running_var"])
    assert hip["num_batches_tracked"] == 0


def _tie_case():
    """4 queries of 4 samples over 10 rows, 8 channels.  Query 0 meets rows 5 and 2, which are identical and dominate (sample 1 before
    sample 2); query 1 is one hit padded three times; query 2 meets row 8, which holds a NaN; query 3 is empty."""
    d = vc.build(((4,), (10,), 4, 8, 0.0))
    d["f"][5] = 10.0
    d["f"][2] = d["f"][5]
    d["xyz"][2] = d["xyz"][5]
    d["f"][3] = 10.0
    d["idx"] = torch.tensor([[7, 5, 2, 7], [3, 3, 3, 3], [8, 9, 8, 8], [0, 0, 0, 0]], dtype=torch.int32)
    d["empty"] = torch.tensor([False, False, False, True])
    d["gamma"] = d["gamma"] * 0.1   # the position branch stays far below the dominating rows
    return d


def test_ties(gpu):
    d = _tie_case()
    hip = _hip_steps(d, gpu, 0.1, True, 1)[0]
    out, gf, go = hip["out"].cpu(), hip["grad_f"].cpu(), d["grad_out"]
    assert bool((out[:2] > 5).all())
    assert torch.equal(gf[5], go[0]) and torch.equal(gf[2], torch.zeros(8)), "a tie goes to the lower sample number"
    assert torch.equal(gf[7], torch.zeros(8))
    assert torch.equal(gf[3], go[1]), "a padded list's gradient lands once"
    assert torch.equal(gf[0], torch.zeros(8)), "an empty query sends no gradient to row 0"


def test_nan_cells(gpu):
    d = _tie_case()
    d["f"][8, 1] = float("nan")
    d["f"][9, 6] = float("nan")
    conv, bn = vc.modules(d, 0.1, True, device=gpu)
    with torch.no_grad():
        out = voxel_pool_fused.voxel_pool_max(*_dev(d, gpu, "f", "xyz", "new_xyz", "idx", "empty"), conv, bn).cpu()
        conv32, bn32 = vc.modules(d, 0.1, True)
        want, _, _ = vc.grouped_pool(d["f"], d["xyz"], d["new_xyz"], d["idx"], d["empty"], conv32, bn32)
    assert torch.equal(torch.isnan(out), torch.isnan(want))
    assert torch.isnan(out).sum() == 2 and bool(torch.isnan(out[2, 1])) and bool(torch.isnan(out[2, 6]))
    assert torch.allclose(out[~torch.isnan(out)], want[~torch.isnan(want)], rtol=1e-4, atol=1e-5)


def test_out_of_range_indices(gpu):
    """Entries N + 5 and -3 behave as rows of zeros (the restatement appends one) and receive no gradient.  Every kernel checks a row
    against [0, N) before it reads: the call stays inside its buffers."""
    ms, ns, s, c, _ = case = ((40,), (30,), 8, 16, 0.2)
    d = vc.build(case)
    live = (~d["empty"]).nonzero().flatten()
    d["idx"][live[0], 1] = ns[0] + 5
    d["idx"][live[1], 0] = -3
    d["idx"][live[2], s - 1] = -3
    _, marg = vc.restated(d, 0.1, True, torch.float64)
    mask = (marg >= vc.MARGIN).float()
    r64, _ = vc.restated(d, 0.1, True, torch.float64, 1, mask)
    r32, _ = vc.restated(d, 0.1, True, torch.float32, 1, mask)
    hip = _hip_steps(d, gpu, 0.1, True, 1, mask)[0]
    for k in FLOATS:
        vc.within(k, hip[k], r32[0][k], r64[0][k])
    assert hip["grad_f"].shape == (ns[0], c) and bool(torch.isfinite(hip["grad_f"]).all())


def test_run_to_run(gpu):
    d = vc.build(vc.CASES["two_samples"])
    a, b = _hip_steps(d, gpu, 0.1, True, 1)[0], _hip_steps(d, gpu, 0.1, True, 1)[0]
    for k in FLOATS:
        assert torch.equal(a[k], b[k]), k


def test_subsets(gpu):
    d, mask, r64, r32 = vc.reference("config", 0.1, True)
    full = _hip_steps(d, gpu, 0.1, True, 1, mask)[0]
    params_only = _hip_steps(d, gpu, 0.1, True, 1, mask, grads=(False, True))[0]
    assert params_only["grad_f"] is None
    for k in ("grad_w", "grad_gamma", "grad_beta"):
        assert torch.equal(params_only[k], full[k]), k
    rows_only = _hip_steps(d, gpu, 0.1, True, 1, mask, grads=(True, False))[0]
    assert rows_only["grad_w"] is None and rows_only["grad_gamma"] is None and rows_only["grad_beta"] is None
    assert torch.equal(rows_only["grad_f"], full["grad_f"])


def test_no_grad_allocates_no_arg(gpu, monkeypatch):
    d = vc.build(vc.CASES["config"])
    conv, bn = vc.modules(d, 0.1, True, device=gpu)
    args = _dev(d, gpu, "f", "xyz", "new_xyz", "idx", "empty")
    made = []
    real = voxel_pool_fused.G.new
    monkeypatch.setattr(voxel_pool_fused.G, "new", lambda like, shape, dtype=torch.float32, fill=None: made.append(dtype) or real(like, shape, dtype, fill))
    with torch.no_grad():
        out = voxel_pool_fused.voxel_pool_max(*args, conv, bn)
    assert out is not None and torch.uint8 not in made
    made.clear()
    voxel_pool_fused.voxel_pool_max(*args, conv, bn)
    assert torch.uint8 in made


def test_forward_memory(gpu):
    ms, ns, s, c, _ = vc.MEMORY_CASE
    d = vc.build(vc.MEMORY_CASE)
    conv, bn = vc.modules(d, 0.1, True, device=gpu)
    args = _dev(d, gpu, "f", "xyz", "new_xyz", "idx", "empty")
    args[0].requires_grad_(True)
    voxel_pool_fused.voxel_pool_max(*args, conv, bn)   # warm-up: the workspace is taken here
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    out = voxel_pool_fused.voxel_pool_max(*args, conv, bn)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    grouped = ms[0] * c * s * 4
    print(f"forward memory: +{rise} bytes, the grouped tensor would be {grouped}")
    assert out.requires_grad and rise < grouped // 4


# ---- the module ------------------------------------------------------------------------------------------------------------------
def _module(gpu, cmid, pool, seed=0):
    torch.manual_seed(seed)
    mod = voxel_pool_modules.NeighborVoxelSAModuleMSG(query_ranges=[[1, 2, 2], [1, 3, 3]], radii=[0.25, 0.4], nsamples=[16, 16],
                                                      mlps=[[8, cmid, 16], [8, cmid, 16]], pool_method=pool)
    with torch.no_grad():   # away from the constant initialisation of the BatchNorms
        for m in mod.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.3)
    return mod.to(gpu)


def _run_module(mod, occ, gpu, fused):
    mod = copy.deepcopy(mod)
    mod.FUSED = fused
    t = {k: v.to(gpu) for k, v in occ.items()}
    out = mod(t["xyz"], t["xyz_batch_cnt"], t["new_xyz"], t["new_xyz_batch_cnt"], t["new_coords"], t["features"], t["vol"])
    (out * t["grad_out"]).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), {n: p.grad for n, p in mod.named_parameters()}, mod.state_dict()


def _lists(mod, occ, gpu):
    t = {k: v.to(gpu) for k, v in occ.items()}
    coords = t["new_coords"][:, [0, 3, 2, 1]].contiguous()
    res = []
    for g in mod.groupers:
        idx, empty = g.query(coords, t["xyz"], t["xyz_batch_cnt"], t["new_xyz"], t["new_xyz_batch_cnt"], t["vol"])
        res.append((idx.cpu(), empty.cpu()))
    return res


@pytest.mark.parametrize("ns,ms", [((300,), (90,)), ((300, 220), (90, 70))])
def test_module(gpu, ns, ms, monkeypatch):
    occ = vc.occupancy(ns, ms)
    mod = _module(gpu, 32, "max_pool")
    lists = _lists(mod, occ, gpu)
    assert all(0 < int(e.sum()) < e.numel() for _, e in lists), "the occupancy should leave some queries empty, not all"
    o64, g64, s64, low = vc.module_restated(mod, occ, lists, torch.float64)
    o32, g32, s32, _ = vc.module_restated(mod, occ, lists, torch.float32)
    assert low >= vc.MARGIN, f"a cell within {vc.MARGIN} of a tie ({low:.1e}): choose another seed"
    calls = []
    real = voxel_pool_fused.voxel_pool_max
    monkeypatch.setattr(voxel_pool_fused, "voxel_pool_max", lambda *a: calls.append(1) or real(*a))
    for fused in (True, False):
        calls.clear()
        out, grads, state = _run_module(mod, occ, gpu, fused)
        assert len(calls) == (2 if fused else 0)
        print(f"module B={len(ns)} FUSED={fused}")
        vc.within("out", out, o32, o64)
        for n in g64:
            vc.within("grad " + n, grads[n], g32[n], g64[n])
        for n, v in s64.items():
            if v.dtype == torch.int64:
                assert int(state[n]) == int(v), n
            else:
                vc.within("state " + n, state[n], s32[n], v)


@pytest.mark.parametrize("cmid,pool", [(6, "max_pool"), (32, "avg_pool")])
def test_module_torch_route_cases(gpu, cmid, pool, monkeypatch):
    """Six channels and avg_pool are not the fused op's: both switches run the torch composition."""
    occ = vc.occupancy((300, 220), (90, 70))
    mod = _module(gpu, cmid, pool)

    def refuse(*a):
        raise AssertionError("the fused op was called")
    monkeypatch.setattr(voxel_pool_fused, "voxel_pool_max", refuse)
    on, off = _run_module(mod, occ, gpu, True), _run_module(mod, occ, gpu, False)
    assert torch.allclose(on[0], off[0], rtol=1e-5, atol=1e-6)
    for n in on[1]:   # (the grouping gradient of the torch route adds with float atomics: last bits may move)
        assert torch.allclose(on[1][n], off[1][n], rtol=1e-4, atol=1e-5), n
    for n, v in on[2].items():
        assert torch.allclose(v.float(), off[2][n].float(), rtol=1e-5, atol=1e-6), n
    lists = _lists(mod, occ, gpu)
    o64, _, _, _ = vc.module_restated(mod, occ, lists, torch.float64, pool)
    o32, _, _, _ = vc.module_restated(mod, occ, lists, torch.float32, pool)
    vc.within("out", on[0], o32, o64)
