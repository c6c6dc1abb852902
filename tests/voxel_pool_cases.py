"""Shared builders of the voxel-pool tests (test_voxel_pool_cpu.py / test_voxel_pool_gpu.py).

The truth is the grouped formulation of the reference's NeighborVoxelSAModuleMSG (voxel_pool_modules.py:108-135), restated here
with plain torch indexing on GLOBAL rows, on the CPU: it never goes through the library.  Run in float64 it is the truth, run in
float32 it is the yardstick: every float comparison is rel_l2(hip, f64) <= max(K * rel_l2(host32, f64), FLOOR) (f64_calibration).
An index outside [0, N) names a row of zeros appended to F and to xyz (the library's rule for such an entry)."""
import functools

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from f64_calibration import FLOOR, K, rel_l2

MARGIN = 1e-5          # float64 margin below which a (query, channel) cell's arg-max / ReLU decision is left out of gradient comparisons
MAX_MASKED = 1e-3      # ... and the share of cells that may be left out
EPS = 1e-5

# name -> (M per sample, N per sample, S, C, share of empty queries)
CASES = {
    "one": ((1,), (3,), 2, 4, 0.0),
    "c12": ((37,), (23,), 5, 12, 0.2),
    "config": ((300,), (150,), 16, 32, 0.2),
    "blocks": ((513,), (200,), 32, 32, 0.2),
    "c128": ((64,), (40,), 16, 128, 0.2),
    "two_samples": ((130, 127), (50, 40), 16, 64, 0.2),
    "all_empty": ((20,), (10,), 16, 32, 1.0),
    "none_empty": ((100,), (60,), 16, 32, 0.0),
}
MEMORY_CASE = ((2048,), (500,), 16, 32, 0.2)


def index_lists(rng, ms, ns, s, empty_share):
    """(idx (M, S) int32 global rows, empty (M) bool) as the voxel query leaves them: k <= S distinct hits of the query's own
    sample, the rest padded with the first hit; an empty query holds zeros and has its mask set."""
    idx, empty = [], []
    lo = 0
    for m_b, n_b in zip(ms, ns):
        for _ in range(m_b):
            if rng.random() < empty_share:
                idx.append(np.zeros(s, np.int32)); empty.append(True)
                continue
            k = int(rng.integers(1, min(s, n_b) + 1))
            hits = lo + rng.choice(n_b, k, replace=False)
            idx.append(np.concatenate([hits, np.full(s - k, hits[0])]).astype(np.int32)); empty.append(False)
        lo += n_b
    return torch.from_numpy(np.stack(idx)), torch.tensor(empty)


def build(case, seed=0):
    """float32 CPU inputs and parameters of one case."""
    ms, ns, s, c, share = case
    rng = np.random.default_rng(seed)
    g = torch.Generator().manual_seed(seed)
    m, n = sum(ms), sum(ns)
    idx, empty = index_lists(rng, ms, ns, s, share)
    return dict(f=torch.randn(n, c, generator=g), xyz=torch.rand(n, 3, generator=g) * 2, new_xyz=torch.rand(m, 3, generator=g) * 2,
                idx=idx, empty=empty, w=torch.randn(c, 3, 1, 1, generator=g) * 0.8, gamma=torch.rand(c, generator=g) + 0.5,
                beta=torch.randn(c, generator=g) * 0.3, running_mean=torch.randn(c, generator=g) * 0.2,
                running_var=torch.rand(c, generator=g) + 0.5, grad_out=torch.randn(m, c, generator=g))


def modules(d, momentum, training, dtype=torch.float32, device="cpu"):
    """The Conv2d(3, C, 1) / BatchNorm2d pair of mlps_pos with the case's parameters and running statistics."""
    c = d["w"].shape[0]
    conv, bn = nn.Conv2d(3, c, 1, bias=False), nn.BatchNorm2d(c, eps=EPS, momentum=momentum)
    with torch.no_grad():
        conv.weight.copy_(d["w"]); bn.weight.copy_(d["gamma"]); bn.bias.copy_(d["beta"])
        bn.running_mean.copy_(d["running_mean"]); bn.running_var.copy_(d["running_var"])
    conv, bn = conv.to(device=device, dtype=dtype), bn.to(device=device, dtype=dtype)
    bn.train(training)
    return conv, bn


def grouped_pool(f, xyz, new_xyz, idx, empty, conv, bn, pool="max_pool"):
    """The module's body between mlps_in and mlps_out on global rows -> (out (M, C), pre (M, C, S) before the ReLU, rows (M, S))."""
    n = f.shape[0]
    rows = idx.long().clone()
    rows[(rows < 0) | (rows >= n)] = n
    fz, xz = torch.cat([f, f.new_zeros(1, f.shape[1])]), torch.cat([xyz, xyz.new_zeros(1, 3)])
    gf = fz[rows].permute(0, 2, 1).clone()                    # (M, C, S)
    gxyz = xz[rows].permute(0, 2, 1) - new_xyz.unsqueeze(-1)   # (M, 3, S)
    gf[empty] = 0
    gxyz[empty] = 0
    pos = bn(conv(gxyz.permute(1, 0, 2).unsqueeze(0)))
    pre = gf.permute(1, 0, 2).unsqueeze(0) + pos               # (1, C, M, S)
    act = F.relu(pre)
    pooled = F.max_pool2d(act, kernel_size=[1, act.size(3)]) if pool == "max_pool" else F.avg_pool2d(act, kernel_size=[1, act.size(3)])
    return pooled.squeeze(-1)[0].t(), pre[0].permute(1, 0, 2), rows


def margins(pre, rows):
    """(M, C) float64 margin of every cell: the distance of the best pre-activation from 0, and - where it is positive - its
    distance from the best candidate of a DIFFERENT row (the query's repeat padding names the winner's own row again)."""
    pre = pre.detach()
    best, arg = pre.max(dim=2)                                                      # (M, C)
    win_row = torch.gather(rows.unsqueeze(1).expand(-1, pre.shape[1], -1), 2, arg.unsqueeze(-1))   # (M, C, 1)
    other = pre.masked_fill(rows.unsqueeze(1) == win_row, float("-inf")).max(dim=2).values
    return torch.where(best > 0, torch.minimum(best, best - other), best.abs())


def restated(d, momentum, training, dtype, steps=1, grad_mask=None):
    """`steps` forward + backward passes of the restatement in `dtype` on the CPU -> list of per-step dicts (out, the gradients,
    the BatchNorm state after the step) and the margins of step 1."""
    conv, bn = modules(d, momentum, training, dtype)
    f = d["f"].to(dtype).clone().requires_grad_(True)   # (a copy: float32 .to(float32) would hand back the shared input itself)
    xyz, new_xyz = d["xyz"].to(dtype), d["new_xyz"].to(dtype)
    res, marg = [], None
    for _ in range(steps):
        for t in (f, conv.weight, bn.weight, bn.bias):
            t.grad = None
        out, pre, rows = grouped_pool(f, xyz, new_xyz, d["idx"], d["empty"], conv, bn)
        if marg is None:
            marg = margins(pre, rows)
        go = d["grad_out"].to(dtype)
        if grad_mask is not None:
            go = go * grad_mask.to(dtype)
        out.backward(go)
        res.append(dict(out=out.detach().clone(), grad_f=f.grad.clone(), grad_w=conv.weight.grad.clone(), grad_gamma=bn.weight.grad.clone(),
                        grad_beta=bn.bias.grad.clone(), running_mean=bn.running_mean.clone(), running_var=bn.running_var.clone(),
                        num_batches_tracked=int(bn.num_batches_tracked)))
    return res, marg


@functools.lru_cache(maxsize=None)
def reference(name, momentum, training, steps=2):
    """(inputs, gradient mask, float64 steps, float32 steps) of a case: computed once, shared by the tests, never modified."""
    d = build(CASES[name] if isinstance(name, str) else name)
    _, marg = restated(d, momentum, training, torch.float64, 1)
    mask = (marg >= MARGIN).to(torch.float32)
    assert float((mask == 0).float().mean()) <= MAX_MASKED, "too many cells within MARGIN of a tie: choose another seed"
    r64, _ = restated(d, momentum, training, torch.float64, steps, mask)
    r32, _ = restated(d, momentum, training, torch.float32, steps, mask)
    return d, mask, r64, r32


def within(what, hip, host32, f64, report=print):
    """The one float comparison of these tests; prints both distances before it judges."""
    d_hip, d_ref = rel_l2(hip, f64), rel_l2(host32, f64)
    bound = max(K * d_ref, FLOOR)
    report(f"  {what:28s} hip {d_hip:.2e}  host32 {d_ref:.2e}  bound {bound:.2e}")
    assert d_hip <= bound, f"{what}: {d_hip:.2e} from float64, the float32 restatement {d_ref:.2e} (bound {bound:.2e})"


# ---- the module: a small synthetic occupancy for the real voxel query -------------------------------------------------------------
def occupancy(ns, ms, seed=0, grid=(4, 40, 40), cin=8):
    """Voxel centres of `ns` occupied voxels per sample in a (Z, Y, X) grid and `ms` queries per sample placed near occupied voxels
    -> dict of CPU tensors in the layout NeighborVoxelSAModuleMSG.forward takes (new_coords as [b, x, y, z])."""
    rng = np.random.default_rng(seed)
    z, y, x = grid
    vs = np.array([0.1, 0.1, 0.2], np.float32)   # x, y, z voxel size
    vol = -np.ones((len(ns), z, y, x), np.int32)
    xyz, new_xyz, new_coords = [], [], []
    lo = 0
    for b, (n_b, m_b) in enumerate(zip(ns, ms)):
        flat = rng.choice(z * y * x, n_b, replace=False)
        cz, cy, cx = flat // (y * x), (flat // x) % y, flat % x
        vol[b, cz, cy, cx] = lo + np.arange(n_b)
        p = (np.stack([cx, cy, cz], 1) + rng.uniform(0.2, 0.8, (n_b, 3))) * vs
        xyz.append(p.astype(np.float32))
        if m_b:
            q = rng.integers(0, n_b, m_b)
            shift = rng.integers(-2, 3, (m_b, 3))
            qc = np.clip(np.stack([cx[q], cy[q], cz[q]], 1) + shift, 0, [x - 1, y - 1, z - 1])
            new_coords.append(np.concatenate([np.full((m_b, 1), b), qc], 1).astype(np.int32))
            new_xyz.append(((qc + 0.5) * vs).astype(np.float32))
        lo += n_b
    g = torch.Generator().manual_seed(seed)
    n, m = sum(ns), sum(ms)
    return dict(xyz=torch.from_numpy(np.concatenate(xyz)), xyz_batch_cnt=torch.tensor(ns, dtype=torch.int32),
                new_xyz=torch.from_numpy(np.concatenate(new_xyz)), new_xyz_batch_cnt=torch.tensor(ms, dtype=torch.int32),
                new_coords=torch.from_numpy(np.concatenate(new_coords)), features=torch.randn(n, cin, generator=g),
                vol=torch.from_numpy(vol), grad_out=torch.randn(m, 1, generator=g))


def module_restated(mod, occ, lists, dtype, pool="max_pool"):
    """NeighborVoxelSAModuleMSG.forward + backward restated on the CPU in `dtype` on a copy of `mod`, with the (idx, empty) pair of
    every grouper given (global rows) -> (out, {parameter: gradient}, state_dict, smallest margin)."""
    import copy
    ref = copy.deepcopy(mod).cpu().to(dtype)
    for b in ref.buffers():   # (num_batches_tracked stays int64)
        assert b.dtype in (dtype, torch.int64)
    feats = occ["features"].to(dtype)
    xyz, new_xyz = occ["xyz"].to(dtype), occ["new_xyz"].to(dtype)
    outs, low = [], float("inf")
    for k, (idx, empty) in enumerate(lists):
        f_in = ref.mlps_in[k](feats.t().unsqueeze(0))[0].t()
        pooled, pre, rows = grouped_pool(f_in, xyz, new_xyz, idx, empty, ref.mlps_pos[k][0], ref.mlps_pos[k][1], pool)
        low = min(low, float(margins(pre, rows).min()))
        outs.append(ref.mlps_out[k](pooled.t().unsqueeze(0))[0].t())
    out = torch.cat(outs, 1)
    (out * occ["grad_out"].to(dtype)).sum().backward()
    return out.detach(), {n: p.grad for n, p in ref.named_parameters()}, ref.state_dict(), low
