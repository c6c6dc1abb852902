#!/usr/bin/env python3
"""Cost of deterministic mode (pcdet.ops.set_deterministic): each backward that adds with float atomics against its fixed-order *_gather
form on random (not hub) inputs, and the reduced FV2P training step (tests/test_fv2p_step_gpu.py: SmallFV2P) with the mode off and on.
Not part of the product or of bench.py.   python tools/det_cost.py [ops|step|all]"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "from-voxel-to-point_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import fv2p_native as _nat  # noqa: E402
import pcdet.ops as ops  # noqa: E402


def timeit(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3  # us


def both(label, fn):
    """fn() runs one backward through the public wrapper; timed with the mode off, then on."""
    t = []
    for on in (False, True):
        ops.set_deterministic(on)
        t.append(timeit(fn))
    ops.set_deterministic(False)
    print(f"{label:58s} atomic {t[0]:9.1f} us   fixed-order {t[1]:9.1f} us   x{t[1] / t[0]:5.2f}", flush=True)


def op_costs():
    from pcdet.ops.pointnet2.pointnet2_batch import pointnet2_utils as pb, fused
    from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils as ps
    from pcdet.ops.roiaware_pool3d import roiaware_pool3d_utils as ru
    from pcdet.models.backbones_3d.pfe.bev_grid_pooling import _BevInterp
    from pcdet.ops.DeformableConvolutionV2PyTorch import DCN
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)

    def grad_of(op, x, grad):
        x = x.detach().requires_grad_(True)
        return lambda: torch.autograd.grad(op(x), x, grad)

    # RoI head grouping (stack): 2 x 32 RoIs x 216 grid points x 16 samples from 2 x 2048 key points, 128 channels
    m, s, c, n = 64 * 216, 16, 128, 4096
    f = torch.randn(n, c, device=dev)
    idx = torch.randint(0, 2048, (m, s), device=dev, dtype=torch.int32, generator=g)
    fc, ic = torch.tensor([2048, 2048], dtype=torch.int32, device=dev), torch.tensor([m // 2, m // 2], dtype=torch.int32, device=dev)
    both(f"group_points stack  M={m} S={s} C={c} N={n}", grad_of(lambda x: ps.GroupingOperation.apply(x, fc, idx, ic), f, torch.randn(m, c, s, device=dev)))
    # batch layouts: 2 samples, 16384 points, 64 channels
    b, c, n = 2, 64, 16384
    f = torch.randn(b, c, n, device=dev)
    gi = torch.randint(0, n, (b, 2048, 32), device=dev, dtype=torch.int32, generator=g)
    both(f"group_points batch  B={b} C={c} N={n} M=2048 S=32", grad_of(lambda x: pb.GroupingOperation.apply(x, gi), f, torch.randn(b, c, 2048, 32, device=dev)))
    gi = torch.randint(0, n, (b, 4096), device=dev, dtype=torch.int32, generator=g)
    both(f"gather_points       B={b} C={c} N={n} M=4096", grad_of(lambda x: pb.GatherOperation.apply(x, gi), f, torch.randn(b, c, 4096, device=dev)))
    ti = torch.randint(0, 4096, (b, n, 3), device=dev, dtype=torch.int32, generator=g)
    tw = torch.rand(b, n, 3, device=dev)
    fk = torch.randn(b, c, 4096, device=dev)
    both(f"three_interpolate batch B={b} C={c} known=4096 queries={n}", grad_of(lambda x: pb.ThreeInterpolate.apply(x, ti, tw), fk, torch.randn(b, c, n, device=dev)))
    # BEV gather of the key points: 2 x 2048 points, 256 x 100 x 88 map (channels first)
    bev = torch.randn(2, 256, 100, 88, device=dev)
    x, y = torch.rand(2, 2048, device=dev) * 87, torch.rand(2, 2048, device=dev) * 99
    both("bev_interp          B=2 C=256 100x88 n=2048", grad_of(lambda t: _BevInterp.apply(t, x, y, True), bev, torch.randn(2, 2048, 256, device=dev)))
    # RoI-aware pooling: 64 RoIs, 6^3 voxels, 128 channels, 4096 points
    for method in ("max", "avg"):
        rois = torch.cat([torch.rand(64, 3, device=dev) * 10, torch.full((64, 3), 4.0, device=dev), torch.zeros(64, 1, device=dev)], 1)
        pts = torch.rand(4096, 3, device=dev) * 12 - 1
        feat = torch.randn(4096, 128, device=dev)
        both(f"roiaware_pool3d {method}  R=64 6^3 C=128 P=4096",
             grad_of(lambda t: ru.RoIAwarePool3dFunction.apply(rois, pts, t, 6, 128, method), feat, torch.randn(64, 6, 6, 6, 128, device=dev)))
    # fused grid set abstraction: 64 RoIs x 216 centres x 16 samples over 128 points
    pp, pc, w2 = torch.randn(64, 128, 64, device=dev), torch.randn(64, 216, 64, device=dev), torch.randn(64, 64, device=dev) / 8
    si = torch.randint(0, 128, (64, 216, 16), device=dev, dtype=torch.int32, generator=g)
    both("sa_grid             R=64 N=128 M=216 S=16 C=64", grad_of(lambda t: fused.sa_grid_max(t, pc, si, w2), pp, torch.randn(64, 216, 64, device=dev)))
    # deformable PS RoI pooling: 128 RoIs, 7 x 7 bins, 4 x 4 samples, 256 channels on 2 x 200 x 176
    data = torch.randn(2, 256, 200, 176, device=dev)
    r = torch.cat([torch.randint(0, 2, (128, 1), device=dev, generator=g).float(), torch.rand(128, 2, device=dev) * 150,
                   torch.rand(128, 2, device=dev) * 150 + 20], 1)
    r[:, 3:5] = torch.maximum(r[:, 3:5], r[:, 1:3] + 4)
    tr = torch.randn(128, 2, 7, 7, device=dev) * 0.1
    conf = (False, 1.0, 256, 1, 7, 7, 4, 0.1)
    out, top = DCN.deform_psroi_pooling_forward(data, r, tr, *conf)
    go = torch.randn_like(out)
    both("deform_psroi_pool   R=128 C=256 7x7 spp=4 2x200x176", lambda: DCN.deform_psroi_pooling_backward(go, data, r, tr, top, *conf))


def step_cost(reps=10):
    from conftest import deterministic_libraries
    from test_fv2p_step_gpu import SmallFV2P, make_inputs
    from fv2p_harness.fv2p_model import FV2PDetector
    dev = torch.device("cuda:0")
    clouds, feats, coords, gt, u = make_inputs(SmallFV2P, 2, 4096)
    args = ([c.to(dev) for c in clouds], feats.to(dev), coords.to(dev), gt.to(dev), u.to(dev))
    torch.manual_seed(0)
    net = FV2PDetector(SmallFV2P).to(dev)
    net.taps = {}

    def step():
        net.zero_grad(set_to_none=True)
        net(*args).backward()
    for label, on in (("off", False), ("on", True), ("off", False), ("on", True)):
        ops.set_deterministic(on)
        with deterministic_libraries():
            us = timeit(step, reps=reps, warm=2)
        print(f"reduced FV2P step (SmallFV2P, batch 2, deterministic libraries), mode {label:3s}: {us / 1e3:8.2f} ms", flush=True)
    ops.set_deterministic(False)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    _nat.lib()
    if what in ("ops", "all"):
        op_costs()
    if what in ("step", "all"):
        step_cost()
