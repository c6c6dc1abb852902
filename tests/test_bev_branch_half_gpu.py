"""GPU: the dense BEV branch on float16 / bfloat16 storage, end to end: 16-bit sparse rows -> dense() -> Conv2d -> BatchNorm2d+ReLU ->
ConvTranspose2d -> BatchNorm2d+ReLU (norm.run_maps) -> bilinear gather at the key points, forward and backward, after .half() /
.bfloat16() and with the network kept in fp32 under torch.autocast with spconv.set_mixed_precision(True).

Every BatchNorm2d shows one fv2p_batchnorm2d_forward_h and one fv2p_batchnorm2d_backward_h, the gather fv2p_bev_interp_fwd_h / _bwd_h; no
tensor on the path is float32 except parameters, statistics and coordinates; the state-dict keys are unchanged.  The output and the
gradients are judged by the criterion of tests/f64_calibration.py against the torch-module run of the same 16-bit network: a float64 host
run is the truth, and the fused run may be at most K times as far from it as the torch run is."""
import contextlib
import copy

import pytest
import torch
import torch.nn as nn

import f64_calibration as cal
import fv2p_native as nat
import pcdet.ops.spconv as spconv
from pcdet.models.backbones_3d.pfe.bev_grid_pooling import interpolate_from_bev_features
from pcdet.ops.spconv import norm

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]
dtype_id = lambda d: str(d).replace("torch.", "")
BATCH, CIN, GRID, KEYS = 2, 8, [2, 16, 16], 64
UNIT = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24}
RANGE, VOXEL = [0.0, 0.0, -1.0, 32.0, 32.0, 1.0], [1.0, 1.0, 1.0]


def _network():
    torch.manual_seed(0)
    net = nn.Sequential(nn.Conv2d(CIN * GRID[0], 16, 3, padding=1, bias=False), nn.BatchNorm2d(16, eps=1e-3, momentum=0.01), nn.ReLU(),
                        nn.ConvTranspose2d(16, 8, 2, stride=2, bias=False), nn.BatchNorm2d(8, eps=1e-3, momentum=0.01), nn.ReLU())
    with torch.no_grad():   # BatchNorm parameters away from their (1, 0) initial values, as in a trained network
        for m in net.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.3, 0.3)
    return net.train()


def _inputs(dtype):
    g = torch.Generator().manual_seed(1)
    cells = torch.randperm(BATCH * GRID[0] * GRID[1] * GRID[2], generator=g)[:300].sort().values
    ind = torch.stack([cells // (GRID[0] * GRID[1] * GRID[2]), cells // (GRID[1] * GRID[2]) % GRID[0], cells // GRID[2] % GRID[1], cells % GRID[2]], 1).int()
    feats = torch.randn(300, CIN, generator=g).to(dtype)
    keys = torch.cat([torch.rand(BATCH, KEYS, 2, generator=g) * 31.0, torch.zeros(BATCH, KEYS, 1)], 2)
    cot = torch.randn(BATCH, KEYS, 8, generator=g).to(dtype)
    return feats, ind, keys, cot


def _gather64(bev, x, y):
    """bilinear_interpolate_torch of the reference in float64: corners clamped to the map, weights from the clamped corners"""
    b, c, h, w = bev.shape
    x0, y0 = torch.floor(x).long(), torch.floor(y).long()
    x1, y1 = (x0 + 1).clamp(0, w - 1), (y0 + 1).clamp(0, h - 1)
    x0, y0 = x0.clamp(0, w - 1), y0.clamp(0, h - 1)
    im = bev.permute(0, 2, 3, 1)
    bi = torch.arange(b).view(b, 1).expand_as(x0)
    wa, wb = (x1.double() - x) * (y1.double() - y), (x1.double() - x) * (y - y0.double())
    wc, wd = (x - x0.double()) * (y1.double() - y), (x - x0.double()) * (y - y0.double())
    return ((im[bi, y0, x0] * wa.unsqueeze(-1) + im[bi, y1, x0] * wb.unsqueeze(-1)) + im[bi, y0, x1] * wc.unsqueeze(-1)) + im[bi, y1, x1] * wd.unsqueeze(-1)


def _truth(net, feats, ind, keys, cot):
    host = copy.deepcopy(net).double().cpu()
    f = feats.double().requires_grad_(True)
    i = ind.long()
    dense = torch.zeros(BATCH, *GRID, CIN, dtype=torch.float64).index_put((i[:, 0], i[:, 1], i[:, 2], i[:, 3]), f).permute(0, 4, 1, 2, 3)
    out = _gather64(host(dense.reshape(BATCH, CIN * GRID[0], GRID[1], GRID[2])), keys[..., 0].double(), keys[..., 1].double())
    out.backward(cot.double())
    res = {name: p.grad.detach() for name, p in host.named_parameters()}
    res["output"], res["input.grad"] = out.detach(), f.grad.detach()
    return res


def _chain(net, feats, ind, keys, cot, gpu, fused, amp_dtype=None):
    """forward + backward on the GPU -> ({"output", "input.grad", parameter gradients}, the dtypes met on the way)"""
    for p in net.parameters():
        p.grad = None
    f = feats.to(gpu).requires_grad_(True)
    ctx = torch.autocast("cuda", dtype=amp_dtype) if amp_dtype is not None else contextlib.nullcontext()
    with ctx:
        dense = spconv.SparseConvTensor(f, ind.to(gpu), GRID, BATCH).dense()
        bev_in = dense.view(BATCH, CIN * GRID[0], GRID[1], GRID[2])
        bev = norm.run_maps(net, bev_in) if fused else net(bev_in)
        out = interpolate_from_bev_features(keys.to(gpu), bev, BATCH, 1, RANGE, VOXEL)
    out.backward(cot.to(gpu).to(out.dtype))
    torch.cuda.synchronize()
    res = {name: p.grad.detach().cpu() for name, p in net.named_parameters()}
    res["output"], res["input.grad"] = out.detach().cpu(), f.grad.detach().cpu()
    return res, dict(dense=dense.dtype, bev=bev.dtype, out=out.dtype, grad=f.grad.dtype)


class _Recorder:
    """fv2p_native.call with the entry points' names and their float32 tensor arguments noted"""

    def __init__(self):
        self.names, self.fp32, self.inner = [], [], nat.call

    def __call__(self, name, *args):
        self.names.append(name)
        self.fp32 += [(name, tuple(a.shape)) for a in args if torch.is_tensor(a) and a.dtype == torch.float32]
        return self.inner(name, *args)


def _judged(net, dtype, gpu, monkeypatch, amp):
    feats, ind, keys, cot = _inputs(dtype)
    truth = _truth(net, feats, ind, keys, cot)
    dev, twin = copy.deepcopy(net).to(gpu), copy.deepcopy(net).to(gpu)
    if not amp:
        dev, twin = dev.to(dtype), twin.to(dtype)
    rec = _Recorder()
    monkeypatch.setattr(nat, "call", rec)
    fused, seen = _chain(dev, feats, ind, keys, cot, gpu, True, dtype if amp else None)
    names, fp32 = list(rec.names), list(rec.fp32)
    del rec.names[:]
    plain, seen_plain = _chain(twin, feats, ind, keys, cot, gpu, False, dtype if amp else None)
    names_plain = list(rec.names)
    monkeypatch.setattr(nat, "call", rec.inner)
    # one forward and one backward launch set per BatchNorm2d, the 16-bit gather and its gradient
    assert names.count("fv2p_batchnorm2d_forward_h") == 2 and names.count("fv2p_batchnorm2d_backward_h") == 2, names
    assert names.count("fv2p_bev_interp_fwd_h") == 1 and names.count("fv2p_bev_interp_bwd_h") == 1, names
    assert not any(n in ("fv2p_batchnorm2d_forward", "fv2p_batchnorm2d_backward", "fv2p_bev_interp_fwd", "fv2p_bev_interp_bwd") for n in names), names
    assert not any("batchnorm2d" in n for n in names_plain), names_plain
    # float32 reaches the library as parameters, statistics ([C]) and coordinates ([B, N]) only
    for name, shape in fp32:
        assert len(shape) <= 2 and (shape in ((16,), (8,)) or shape == (BATCH, KEYS)), (name, shape)
    assert all(v == dtype for v in seen.values()), seen
    for name, p in dev.named_parameters():
        assert p.grad.dtype == p.dtype == (torch.float32 if amp else dtype), name
    assert list(dev.state_dict()) == list(net.state_dict())
    for (k, a), b in zip(dev.state_dict().items(), twin.state_dict().values()):
        if "num_batches_tracked" in k:
            assert int(a) == int(b) == 1, k
        if "running" in k:
            # Both moved by momentum 0.01 towards the statistics of THEIR OWN 16-bit activations, which differ between the two runs by a
            # few roundings of the format (u |x|, |x| within 8 here; torch also sums in fp32): 0.01 * 16 u, plus two roundings of the
            # buffers' own format.  A missing or doubled update is 0.01 * var ~ 1e-2.
            tol = 0.16 * UNIT[dtype] + 2 * UNIT[a.dtype]
            assert torch.allclose(a.float(), b.float(), rtol=tol, atol=tol), k
    rows, bad = cal.compare(fused, plain, truth, lambda n: "output" if n == "output" else "gradients")
    print(cal.report(rows, "distance to the float64 run: fused 16-bit op (hip) against torch's modules on the same 16-bit network (h32)"))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_branch_after_half_or_bfloat16(gpu, monkeypatch, dtype):
    _judged(_network(), dtype, gpu, monkeypatch, amp=False)


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_branch_in_fp32_under_autocast_with_mixed_precision(gpu, monkeypatch, dtype):
    spconv.set_mixed_precision(True)
    try:
        _judged(_network(), dtype, gpu, monkeypatch, amp=True)
    finally:
        spconv.set_mixed_precision(False)


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_autocast_without_mixed_precision_takes_torchs_modules(gpu, monkeypatch, dtype):
    feats, ind, keys, cot = _inputs(dtype)
    net = _network().to(gpu)
    rec = _Recorder()
    monkeypatch.setattr(nat, "call", rec)
    assert not spconv.ops.mixed_precision()
    res, _ = _chain(net, feats, ind, keys, cot, gpu, True, dtype)
    monkeypatch.setattr(nat, "call", rec.inner)
    assert not any("batchnorm2d" in n for n in rec.names), rec.names
    assert all(torch.isfinite(v.float()).all() for v in res.values())
