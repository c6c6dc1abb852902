"""The dense BEV branch with its (BatchNorm2d, ReLU) pairs as the fused op (KERNEL_GLUE on) against the same modules run by torch
(KERNEL_GLUE off), judged by the float64-calibrated criterion of tests/f64_calibration.py: a third run of the same network on the host
in float64 is the truth, and the fused run may be at most K times as far from it as the torch run is - for the output and for every
parameter gradient (per parameter, as the typical parameter and pooled; FLOOR / PER_PARAM where both runs are closer than fp32 means).
Each float32 run is measured against the float64 run that takes that run's own ReLU decisions (see _three_runs)."""
import copy
import statistics

import pytest
import torch
import torch.nn as nn

import f64_calibration as cal
import fv2p_native
from fv2p_harness import fv2p_model, mgaf_model

pytestmark = pytest.mark.gpu


def _run(net, call, x, w):
    """forward + backward of call(net, x) with the fixed cotangent w -> {"output": y, name: grad}."""
    for p in net.parameters():
        p.grad = None
    xin = x.clone().requires_grad_(True)
    y = call(net, xin)
    (y * w).sum().backward()
    out = {name: p.grad.detach().cpu() for name, p in net.named_parameters()}
    out["output"] = y.detach().cpu()
    out["input.grad"] = xin.grad.detach().cpu()
    return out


def _relus(net):
    return [m for m in net.modules() if isinstance(m, nn.ReLU)]


def _truth(net, call, x, w, masks):
    """The float64 host run.  masks = None: its own ReLUs, whose masks are returned too; otherwise every ReLU (in call order) multiplies
    by the given mask - the ReLU decisions of the float32 run under judgement."""
    host = copy.deepcopy(net).double()
    seen, it = [], iter(masks or [])
    for m in _relus(host):
        if masks is None:
            m.register_forward_hook(lambda mod, i, o: seen.append(o.detach() > 0))
        else:
            m.forward = lambda t, it=it: t * next(it).double()
    return _run(host, call, x.double(), w.double()), seen


def _three_runs(net, call, shape, gpu, monkeypatch, expect_pairs):
    """ReLU decisions.  A pre-activation within rounding of zero takes either side of its ReLU in a float32 run, and one such element in
    the last layers moves every upstream gradient by ~ 1 / sqrt(elements) (tests/f64_calibration.py, `ReLU decisions`): 7e-3 at these map
    sizes, in whichever of the two float32 runs it happens to fall (it changed sides between two machines).  As in tests/test_bn2d_gpu.py
    each float32 run is therefore judged against the float64 run WITH ITS OWN masks, and its masks may differ from the float64 run's own
    in at most 0.1 % of the elements."""
    from conftest import deterministic_libraries
    from pcdet.ops.spconv import norm
    torch.manual_seed(0)
    net.train()
    with torch.no_grad():   # BatchNorm parameters away from their (1, 0) initial values, as in a trained network
        for m in net.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.3, 0.3)
    x = torch.randn(shape)
    y64 = call(copy.deepcopy(net).double(), x.double())
    w = torch.randn(y64.shape)
    _, masks64 = _truth(net, call, x, w, None)
    dev = copy.deepcopy(net).to(gpu)
    twin = copy.deepcopy(net).to(gpu)
    ext = fv2p_native.torch_ext()
    assert ext is not None
    masks_fused, masks_plain = [], []
    fused_op = norm.batch_norm2d_relu

    def recording(bn, t, relu_module=None):
        y = fused_op(bn, t, relu_module)
        if y is not None and relu_module is not None:
            masks_fused.append((y.detach() > 0).cpu())
        return y
    for m in _relus(twin):
        m.register_forward_hook(lambda mod, i, o: masks_plain.append((o.detach() > 0).cpu()))
    with deterministic_libraries():
        ext.record_entry_points(True)
        try:
            monkeypatch.setattr(norm, "batch_norm2d_relu", recording)
            fused = _run(dev, call, x.to(gpu), w.to(gpu))
            torch.cuda.synchronize()
            names = list(ext.entry_points())
            monkeypatch.setattr(norm, "batch_norm2d_relu", fused_op)
            monkeypatch.setattr(fv2p_model, "KERNEL_GLUE", False)
            plain = _run(twin, call, x.to(gpu), w.to(gpu))
            torch.cuda.synchronize()
            names_plain = list(ext.entry_points())
        finally:
            ext.record_entry_points(False)
    assert names.count("fv2p_batchnorm2d_forward") == expect_pairs and names.count("fv2p_batchnorm2d_backward") == expect_pairs, names
    assert not any("batchnorm2d" in n for n in names_plain), names_plain
    assert len(masks_fused) == len(masks_plain) == len(masks64) == expect_pairs
    total = sum(m.numel() for m in masks64)
    for name, masks in (("fused", masks_fused), ("torch", masks_plain)):
        flips = sum(int((a != b).sum()) for a, b in zip(masks, masks64))
        print(f"{name}: {flips} of {total} ReLU decisions differ from the float64 run's")
        assert flips <= 1e-3 * total, f"{name}: {flips} of {total} ReLU decisions differ from the float64 run's"
    # running statistics moved the same way by both
    for (k, a), b in zip(dev.state_dict().items(), twin.state_dict().values()):
        if "running" in k:
            assert torch.allclose(a, b, rtol=1e-5, atol=1e-7), k
        if "num_batches_tracked" in k:
            assert int(a) == int(b) == 1, k
    assert list(dev.state_dict()) == list(net.state_dict())
    truth_f, _ = _truth(net, call, x, w, masks_fused)
    truth_p, _ = _truth(net, call, x, w, masks_plain)
    # the criterion of f64_calibration.compare, with each run's distance taken to the float64 run that made its ReLU decisions
    d_f, d_p = cal.distances(fused, truth_f), cal.distances(plain, truth_p)
    assert set(d_f) == set(d_p) and d_f
    bad = []
    for group in ("output", "gradients"):
        names_g = [n for n in d_f if (n == "output") == (group == "output")]
        fmed, pmed = statistics.median(d_f[n] for n in names_g), statistics.median(d_p[n] for n in names_g)
        fpool, ppool = cal.pooled(fused, truth_f, names_g), cal.pooled(plain, truth_p, names_g)
        print(f"{group:10s} n={len(names_g):3d} | fused med {fmed:.1e} torch med {pmed:.1e} | fused pooled {fpool:.1e} torch pooled {ppool:.1e} | "
              f"fused max {max(d_f[n] for n in names_g):.1e} torch max {max(d_p[n] for n in names_g):.1e}")
        if fmed > max(cal.K * pmed, cal.FLOOR):
            bad.append(f"{group}: median {fmed:.2e} against torch's {pmed:.2e}")
        if fpool > max(cal.K * ppool, cal.FLOOR):
            bad.append(f"{group}: pooled {fpool:.2e} against torch's {ppool:.2e}")
        for n in names_g:
            bound = max(cal.K * d_p[n], 2.0 * cal.K * ppool, cal.PER_PARAM)
            if d_f[n] > bound or d_f[n] > cal.WIRING:
                bad.append(f"{n}: {d_f[n]:.2e} against torch's {d_p[n]:.2e} (bound {bound:.2e})")
    assert not bad, "\n".join(bad)


def test_bev_backbone_fused_against_torch(gpu, monkeypatch):
    net = fv2p_model.BEVBackbone(fv2p_model.FV2PConfig, 256)
    _three_runs(net, lambda m, x: m(x), (2, 256, 16, 12), gpu, monkeypatch, expect_pairs=14)


def test_mgaf_bev_block_and_head_fused_against_torch(gpu, monkeypatch):
    """MGAF's second BEV block (through the same _block its backbone calls) and one convolutional head of its centre head."""
    cfg = mgaf_model.MGAFConfig
    block = mgaf_model.DCNBEVBackbone(cfg, 256).blocks[1]
    head = mgaf_model.CenterAFHead(cfg, 128).heads["hm"]
    net = nn.ModuleDict({"block": block, "head": head})

    def call(m, x):
        h = fv2p_model.BEVBackbone._block(m["block"], x)
        return fv2p_model.run_maps(m["head"], h)
    _three_runs(net, call, (2, 128, 16, 12), gpu, monkeypatch, expect_pairs=7)
