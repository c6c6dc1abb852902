"""The multi-head 1x1 convolution of the anchor head (pcdet.ops.spconv.head, csrc/head1x1.hip) against float64.

Reference: the three F.conv2d calls in float64 on the same inputs, outputs permuted to [B, H * W, c_k]; gradients by autograd through
that float64 form with a random upstream gradient per head.  Bound, per tensor: E = max |torch's own fp32 conv2d path - float64| is
measured first and the op may be off by 2 E + 1e-6 (the convention of tests/test_roi_glue_gpu.py: the bound comes from the fp32
reference, never from the kernel under test).  Every E and every error of the op is printed before it is asserted.

Shapes are the smallest at which the kernels can go wrong: a single position (a); a channel tail and 35 positions per sample, so that
tiles cross the sample boundary (b); odd everything and sum c_k = 20 padded to 32 (c); the real K depth on a small map, 16-byte
accesses (d); a single head (e); sum c_k = 64 exactly (f)."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import fv2p_native as _nat
from fv2p_harness import fv2p_model as fm
from pcdet.ops.spconv import head as H

pytestmark = pytest.mark.gpu

CASES = {          # B, Cin, H, W, heads
    "a": (1, 4, 1, 1, (6, 42, 12)),
    "b": (2, 20, 5, 7, (6, 42, 12)),
    "c": (3, 33, 9, 13, (2, 14, 4)),
    "d": (1, 512, 24, 20, (6, 42, 12)),
    "e": (2, 64, 17, 16, (1,)),
    "f": (2, 64, 17, 16, (16, 48)),
}


def position_major(y):
    return y.permute(0, 2, 3, 1).reshape(y.shape[0], -1, y.shape[1])


def conv_path(x, ws, bs, gs):
    """The three F.conv2d calls in the dtype and on the device of x -> (outputs, dx, dws, dbs)."""
    x = x.detach().requires_grad_(True)
    ws = [w.detach().requires_grad_(True) for w in ws]
    bs = [b.detach().requires_grad_(True) for b in bs]
    outs = [position_major(F.conv2d(x, w, b)) for w, b in zip(ws, bs)]
    grads = torch.autograd.grad(outs, [x] + ws + bs, gs)
    k = len(ws)
    return [o.detach() for o in outs], grads[0], list(grads[1:1 + k]), list(grads[1 + k:])


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs, the float64 result and the per-tensor bounds 2 E + 1e-6 of one case: computed once, shared, never modified."""
    b, cin, h, w, heads = CASES[name]
    torch.manual_seed(sum(map(ord, name)) + cin)
    mods = [nn.Conv2d(cin, ck, 1) for ck in heads]
    for m in mods:
        nn.init.normal_(m.bias, std=0.5)
    mods = [m.cuda() for m in mods]
    x = torch.randn(b, cin, h, w, device="cuda")
    gs = [torch.randn(b, h * w, ck, device="cuda") for ck in heads]
    ws, bs = [m.weight for m in mods], [m.bias for m in mods]
    ref = conv_path(x.double().cpu(), [t.double().cpu() for t in ws], [t.double().cpu() for t in bs], [g.double().cpu() for g in gs])
    t32 = conv_path(x, ws, bs, gs)
    flat = lambda r: list(r[0]) + [r[1]] + list(r[2]) + list(r[3])
    names = [f"y{k}" for k in range(len(heads))] + ["dx"] + [f"dw{k}" for k in range(len(heads))] + [f"db{k}" for k in range(len(heads))]
    refs = dict(zip(names, flat(ref)))
    bounds = {}
    for n, t in zip(names, flat(t32)):
        e = (t.double().cpu() - refs[n]).abs().max().item()
        bounds[n] = 2 * e + 1e-6
        print(f"case {name} {n}: E(torch fp32) = {e:.3e}")
    return dict(mods=mods, x=x, gs=gs, refs=refs, bounds=bounds, heads=heads)


def fused(mods, x, gs, map_grad=True, param_grad=True):
    """The op on (a copy of) the modules -> dict of tensors under the names of case()['refs'] (None where no gradient was asked for)."""
    mods = [copy.deepcopy(m).requires_grad_(param_grad) for m in mods]
    x = x.detach().clone().requires_grad_(map_grad)
    ys = H.multi_conv1x1(mods, x)
    assert ys is not None, "the fused route declined a case it must take"
    torch.autograd.backward(ys, gs)
    out = {f"y{k}": y.detach() for k, y in enumerate(ys)}
    out["dx"] = x.grad
    for k, m in enumerate(mods):
        out[f"dw{k}"], out[f"db{k}"] = m.weight.grad, m.bias.grad
    return out


def check(name, got, keys=None):
    c = case(name)
    bad = []
    for n in (keys or c["refs"]):
        ref = c["refs"][n]
        assert got[n] is not None and got[n].shape == ref.shape and got[n].is_contiguous(), (n, None if got[n] is None else got[n].shape, ref.shape)
        err = (got[n].double().cpu() - ref).abs().max().item()
        print(f"case {name} {n}: op error {err:.3e}, bound {c['bounds'][n]:.3e}")
        if not err <= c["bounds"][n]:
            bad.append((n, err, c["bounds"][n]))
    assert not bad, bad


@pytest.mark.parametrize("name", list(CASES))
def test_matches_float64(gpu, name):
    c = case(name)
    check(name, fused(c["mods"], c["x"], c["gs"]))


class _Recorder:
    """fv2p_native.call with the names of the entry points recorded."""

    def __init__(self, monkeypatch):
        self.names, real = [], _nat.call
        monkeypatch.setattr(_nat, "call", lambda name, *a: (self.names.append(name), real(name, *a))[1])


@pytest.mark.parametrize("name", ["b", "d"])
def test_frozen_map_skips_the_data_kernel(gpu, monkeypatch, name):
    c = case(name)
    rec = _Recorder(monkeypatch)
    got = fused(c["mods"], c["x"], c["gs"], map_grad=False)
    assert got["dx"] is None
    assert "fv2p_head1x1_backward_weights" in rec.names and "fv2p_head1x1_backward_data" not in rec.names, rec.names
    check(name, got, [n for n in c["refs"] if n != "dx"])


@pytest.mark.parametrize("name", ["b", "d"])
def test_frozen_weights_skip_the_weight_kernel(gpu, monkeypatch, name):
    c = case(name)
    rec = _Recorder(monkeypatch)
    got = fused(c["mods"], c["x"], c["gs"], param_grad=False)
    assert all(got[n] is None for n in c["refs"] if n.startswith(("dw", "db")))
    assert "fv2p_head1x1_backward_data" in rec.names and "fv2p_head1x1_backward_weights" not in rec.names, rec.names
    check(name, got, [n for n in c["refs"] if n.startswith("y") or n == "dx"])


@pytest.mark.parametrize("name", ["c", "d"])
def test_weight_and_bias_gradients_are_bit_identical_over_two_runs(gpu, name):
    c = case(name)
    one, two = fused(c["mods"], c["x"], c["gs"]), fused(c["mods"], c["x"], c["gs"])
    for n in c["refs"]:
        assert torch.equal(one[n], two[n]), n


class _SubConv(nn.Conv2d):
    pass


def _fall_through_cases():
    torch.manual_seed(5)
    x = torch.randn(2, 64, 17, 16, device="cuda")
    conv = lambda ck, k=1, cls=nn.Conv2d: cls(64, ck, k, padding=k // 2).cuda()
    return {
        "fp16 map": ([conv(6).half(), conv(42).half()], x.half()),
        "channels-last map": ([conv(6), conv(42)], x.contiguous(memory_format=torch.channels_last)),
        "3x3 kernel": ([conv(6), conv(12, 3)], x),
        "65 columns": ([conv(16), conv(49)], x),
        "Conv2d subclass": ([conv(6), conv(12, cls=_SubConv)], x),
    }


@pytest.mark.parametrize("which", ["fp16 map", "channels-last map", "3x3 kernel", "65 columns", "Conv2d subclass"])
def test_fall_through_calls_the_modules(gpu, monkeypatch, which):
    from conftest import deterministic_libraries
    mods, x = _fall_through_cases()[which]
    rec = _Recorder(monkeypatch)
    assert not H.fusable(mods, x) and H.multi_conv1x1(mods, x) is None
    with deterministic_libraries(), torch.no_grad():
        got = H.run_heads(mods, x)
        want = [position_major(m(x)) for m in mods]
    assert not any(n.startswith("fv2p_head1x1") for n in rec.names), rec.names
    for g, w_ in zip(got, want):
        assert g.dtype == x.dtype and torch.equal(g, w_)


def test_plain_case_takes_the_kernels(gpu, monkeypatch):
    """The counterpart of the fall-through cases: the same shape with plain modules runs the op (and not the modules)."""
    torch.manual_seed(5)
    x = torch.randn(2, 64, 17, 16, device="cuda")
    mods = [nn.Conv2d(64, 6, 1).cuda(), nn.Conv2d(64, 42, 1).cuda()]
    rec = _Recorder(monkeypatch)
    assert H.fusable(mods, x)
    H.run_heads(mods, x)
    assert rec.names == ["fv2p_head1x1_forward"], rec.names


# ------------------------------------------------------------------------------------------------------------------- head level
class SmallCfg(fm.FV2PConfig):
    """A 16 x 12 BEV map (grid_size / 8) with the cell size of the KITTI config."""
    grid_size = (96, 128, 40)
    point_cloud_range = (0.0, -25.6, -3.0, 38.4, 25.6, 1.0)


class _glue:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.was, fm.KERNEL_GLUE = fm.KERNEL_GLUE, self.on

    def __exit__(self, *a):
        fm.KERNEL_GLUE = self.was


def _head_run(head, feat, gt, glue):
    feat = feat.detach().clone().requires_grad_(True)
    params = [p for m in (head.conv_cls, head.conv_box, head.conv_dir_cls) for p in (m.weight, m.bias)]
    with _glue(glue):
        loss, cls, props = head(feat, gt)
        grads = torch.autograd.grad(loss, [feat] + params)
    out = {"loss": loss.detach(), "cls": cls, "proposals": props, "dfeat": grads[0]}
    for n, g in zip(("dw_cls", "db_cls", "dw_box", "db_box", "dw_dir", "db_dir"), grads[1:]):
        out[n] = g
    return out


def test_anchor_head_fused_route_against_the_modules(gpu, monkeypatch):
    """AnchorHead on a [2, 512, 16, 12] map: loss, proposals, parameter and map gradients of the fused route (KERNEL_GLUE on) against
    the modules (KERNEL_GLUE off), each within 2 E + 1e-6 of a float64 copy of the head (on the CPU), E = the error of the KERNEL_GLUE-off fp32 head."""
    from conftest import deterministic_libraries
    torch.manual_seed(3)
    head = fm.AnchorHead(SmallCfg, 512).cuda()
    feat = torch.randn(2, 512, 16, 12, device="cuda")
    gt = torch.zeros(2, 6, 8, device="cuda")
    boxes = [[[10.0, 3.0, -1.0, 3.9, 1.6, 1.56, 0.3, 1], [25.0, -12.0, -0.9, 4.1, 1.7, 1.5, 1.4, 1], [18.0, 9.0, -0.6, 0.8, 0.6, 1.73, 0.1, 2],
              [30.0, 0.0, -0.6, 1.76, 0.6, 1.73, 2.0, 3]],
             [[6.0, -5.0, -1.0, 3.7, 1.6, 1.5, -0.4, 1], [20.0, 15.0, -0.6, 0.9, 0.7, 1.7, 0.9, 2], [33.0, -20.0, -0.6, 1.7, 0.6, 1.7, 1.6, 3],
              [12.0, 20.0, -1.0, 4.0, 1.6, 1.6, 3.0, 1]]]
    gt[:, :4] = torch.tensor(boxes, device="cuda")
    with deterministic_libraries():
        ref = _head_run(copy.deepcopy(head).double().cpu(), feat.double().cpu(), gt.double().cpu(), False)
        mod = _head_run(head, feat, gt, False)
        rec = _Recorder(monkeypatch)
        got = _head_run(head, feat, gt, True)
    assert {"fv2p_head1x1_forward", "fv2p_head1x1_backward_data", "fv2p_head1x1_backward_weights"} <= set(rec.names), rec.names
    bad = []
    for n, r in ref.items():
        e = (mod[n].double().cpu() - r).abs().max().item()
        err = (got[n].double().cpu() - r).abs().max().item()
        gap = (got[n] - mod[n]).abs().max().item()
        print(f"head {n}: E(modules fp32) = {e:.3e}, fused error {err:.3e}, bound {2 * e + 1e-6:.3e}, fused - modules {gap:.3e}")
        if not err <= 2 * e + 1e-6:
            bad.append((n, err, 2 * e + 1e-6))
    assert not bad, bad
