"""CPU: the 16-bit BatchNorm2d (+ReLU) and bilinear-gather entry points exist and are declared, their workspace queries are monotone,
the dtype checks answer before anything else (so they can be reached without a GPU), and `fusable2d16` / `batch_norm2d_relu16` decline
every situation the 16-bit op does not cover - checked on host tensors with a stand-in for `is_cuda`, as test_bn2d_cpu.py does."""
import ctypes
import os

import torch
import torch.nn as nn

import fv2p_native as nat
import pcdet.ops.spconv as spconv
from pcdet.ops.spconv import norm

SYMBOLS = ["fv2p_batchnorm2d_h_ws_bytes", "fv2p_batchnorm2d_forward_h", "fv2p_batchnorm2d_apply_h", "fv2p_batchnorm2d_backward_h",
           "fv2p_bev_interp_h_ws_bytes", "fv2p_bev_interp_fwd_h", "fv2p_bev_interp_bwd_h_ws_bytes", "fv2p_bev_interp_bwd_h",
           "fv2p_transpose_batched_h"]
EINVAL = -1


def test_symbols_are_exported_and_declared():
    raw = ctypes.CDLL(nat.LIB_PATH)
    declared = set(nat.declared_symbols())
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fv2p_ops.h")).read()
    for name in SYMBOLS:
        assert hasattr(raw, name), name
        assert name in declared, name
        assert name + "(" in header, name


def test_batchnorm_ws_bytes_is_monotone_and_steps_at_the_chunk():
    ws = lambda n, c, hw: nat.call("fv2p_batchnorm2d_h_ws_bytes", n, c, hw)
    C = norm.BN2D_CHUNK16
    assert ws(1, 1, 1) > 0
    for n, c, hw in [(1, 1, 1), (2, 5, 35), (3, 128, 200 * 176), (3, 256, 100 * 88)]:
        here = ws(n, c, hw)
        assert ws(n + 1, c, hw) >= here and ws(n, c + 1, hw) >= here and ws(n, c, hw + 1) >= here
        assert ws(4 * n, c, hw) >= here and ws(n, 4 * c, hw) >= here and ws(n, c, 4 * hw + C) >= here
    # one pair of doubles per (sample, channel, chunk): the size steps exactly where a plane needs one more chunk
    assert ws(64, 64, C) == ws(64, 64, 1) < ws(64, 64, C + 1) == ws(64, 64, 2 * C) < ws(64, 64, 2 * C + 1)
    # the fp64 partials and the counter copy only: nothing of the map's size
    assert 3 * 256 * 9 * 16 <= ws(3, 256, 200 * 176) < 3 * 256 * 9 * 16 + 4096
    assert ws(0, 1, 1) == 0 and ws(1, 0, 1) == 0 and ws(1, 1, 0) == 0
    assert ws(1 << 20, 1 << 10, 1) == 0    # more workgroups than a launch takes


def test_bev_ws_bytes_are_monotone():
    fwd = lambda b, c, h, w, cf: nat.call("fv2p_bev_interp_h_ws_bytes", b, c, h, w, cf)
    bwd = lambda b, c, h, w, cf, n: nat.call("fv2p_bev_interp_bwd_h_ws_bytes", b, c, h, w, cf, n)
    assert fwd(3, 256, 200, 176, 1) == 3 * 256 * 200 * 176 * 2 and fwd(3, 256, 200, 176, 0) == 0
    for b, c, h, w in [(1, 1, 1, 1), (2, 7, 5, 6), (3, 256, 200, 176)]:
        for cf in (0, 1):
            here = fwd(b, c, h, w, cf)
            assert fwd(b + 1, c, h, w, cf) >= here and fwd(b, c + 1, h, w, cf) >= here and fwd(b, c, h + 1, w, cf) >= here
            for n in (0, 1, 64, 2048):
                here = bwd(b, c, h, w, cf, n)
                assert here > 0
                assert bwd(b + 1, c, h, w, cf, n) >= here and bwd(b, c + 1, h, w, cf, n) >= here and bwd(b, c, h, w + 1, cf, n) >= here
                assert bwd(b, c, h, w, cf, n + 1) >= here and bwd(b, c, h, w, cf, 4 * n + 33) >= here
            assert bwd(b, c, h, w, 1, 64) >= bwd(b, c, h, w, 0, 64) + b * c * h * w * 2   # the 16-bit staging gradient
    assert fwd(0, 1, 1, 1, 1) == 0 and fwd(1, 0, 1, 1, 1) == 0 and fwd(1, 1, 0, 1, 1) == 0 and fwd(1, 1, 1, 0, 1) == 0
    assert bwd(0, 1, 1, 1, 1, 4) == 0 and bwd(1, 1, 1, 0, 0, 4) == 0 and bwd(1, 1, 1, 1, 0, -1) == 0


def test_bad_dtypes_are_refused_first():
    lib = nat.lib()
    for dt, pd in [(0, 0), (3, 0), (1, 2), (2, 1), (1, 3)]:
        assert lib.fv2p_batchnorm2d_forward_h(None, 1, 1, 4, 1e-3, 0.1, None, None, 1, None, None, None, None, None, None, dt, pd, None, 0,
                                              None) == EINVAL
        assert "batchnorm2d_forward_h" in nat.last_error() and "dtype" in nat.last_error()
        assert lib.fv2p_batchnorm2d_apply_h(None, 1, 1, 4, None, None, None, None, 1, None, dt, pd, None) == EINVAL
        assert "batchnorm2d_apply_h" in nat.last_error() and "dtype" in nat.last_error()
        assert lib.fv2p_batchnorm2d_backward_h(None, None, 1, 1, 4, None, None, None, None, 1, 1, None, None, None, dt, pd, None, 0, None) == EINVAL
        assert "batchnorm2d_backward_h" in nat.last_error() and "dtype" in nat.last_error()
    for dt in (0, 3):
        assert lib.fv2p_bev_interp_fwd_h(None, 1, 1, 1, 1, 1, None, None, 1, None, dt, None, 0, None) == EINVAL
        assert "bev_interp_fwd_h" in nat.last_error() and "dtype" in nat.last_error()
        assert lib.fv2p_bev_interp_bwd_h(None, 1, 1, 1, 1, 1, None, None, 1, None, dt, None, 0, None) == EINVAL
        assert "bev_interp_bwd_h" in nat.last_error() and "dtype" in nat.last_error()
    # a good dtype reaches the next check
    assert lib.fv2p_batchnorm2d_forward_h(None, 1, 1, 4, 1e-3, 0.1, None, None, 1, None, None, None, None, None, None, 1, 0, None, 0, None) == EINVAL
    assert "null" in nat.last_error()
    assert lib.fv2p_batchnorm2d_backward_h(None, None, 0, 1, 4, None, None, None, None, 1, 1, None, None, None, 2, 2, None, 0, None) == EINVAL
    assert "n=0" in nat.last_error()
    assert lib.fv2p_transpose_batched_h(None, 1, 4, 4, None, None) == EINVAL


class _AsCuda(torch.Tensor):
    """A host tensor that answers is_cuda = True: lets the wrapper's later conditions be reached without a GPU."""

    @property
    def is_cuda(self):
        return True


def _as_cuda(t):
    return t.as_subclass(_AsCuda)


def _bn(c=8, dtype=torch.float32, **kw):
    """A BatchNorm2d whose parameters and statistics answer is_cuda = True (and have `dtype`)."""
    bn = nn.BatchNorm2d(c, **kw)
    for k, v in list(bn._parameters.items()):
        if v is not None:
            bn._parameters[k] = _as_cuda(v.detach().to(dtype))
    for k in ("running_mean", "running_var"):
        if bn._buffers.get(k) is not None:
            bn._buffers[k] = _as_cuda(bn._buffers[k].to(dtype))
    return bn


def test_wrapper_declines_every_uncovered_case_on_host_tensors():
    relu = nn.ReLU()
    x = torch.randn(2, 8, 4, 4).half()
    xc = _as_cuda(x)
    assert norm.batch_norm2d_relu16(nn.BatchNorm2d(8).half(), x, relu) is None     # a host tensor
    assert not norm.fusable2d16(_bn(), relu, x)
    assert not norm.fusable2d16(nn.BatchNorm2d(8), relu, xc)                        # parameters not on the GPU
    for dt in (torch.float16, torch.bfloat16):
        xd = _as_cuda(x.to(dt))
        assert norm.fusable2d16(_bn(), relu, xd) and norm.fusable2d16(_bn(), None, xd)       # fp32 parameters ...
        assert norm.fusable2d16(_bn(dtype=dt), relu, xd)                                      # ... or x's dtype ...
        assert norm.fusable2d16(_bn(affine=False), relu, xd) and norm.fusable2d16(_bn(affine=False, track_running_stats=False), relu, xd)
        other = torch.bfloat16 if dt == torch.float16 else torch.float16
        assert not norm.fusable2d16(_bn(dtype=other), relu, xd)                               # ... and no other
        assert not norm.fusable2d16(_bn(dtype=torch.float64), relu, xd)
        mixed = _bn()
        mixed._buffers["running_var"] = _as_cuda(mixed.running_var.to(dt))
        assert not norm.fusable2d16(mixed, relu, xd)                                          # mixed formats
        assert not norm.fusable2d(_bn(), relu, xd) and not norm.fusable2d(_bn(dtype=dt), relu, xd)   # the fp32 op still declines
    bn = _bn()
    assert not norm.fusable2d16(bn, relu, _as_cuda(x.float())) and not norm.fusable2d16(bn, relu, _as_cuda(x.double()))   # dtype

    class MyBn(nn.BatchNorm2d):
        pass
    assert not norm.fusable2d16(MyBn(8, affine=False, track_running_stats=False), relu, xc)   # type(bn) is not nn.BatchNorm2d
    assert not norm.fusable2d16(nn.BatchNorm1d(8, affine=False, track_running_stats=False), relu, xc)
    hooked = _bn()
    hooked.register_forward_hook(lambda m, i, o: None)
    assert not norm.fusable2d16(hooked, relu, xc)                                   # hooks
    pre = _bn()
    pre.register_forward_pre_hook(lambda m, i: None)
    assert not norm.fusable2d16(pre, relu, xc)
    patched = _bn()
    patched.forward = lambda t: t
    assert not norm.fusable2d16(patched, relu, xc)                                  # forward replaced on the instance
    hrelu = nn.ReLU()
    hrelu.register_forward_hook(lambda m, i, o: None)
    assert not norm.fusable2d16(bn, hrelu, xc)
    prelu = nn.ReLU()
    prelu.forward = lambda t: t
    assert not norm.fusable2d16(bn, prelu, xc)
    assert not norm.fusable2d16(bn, nn.ReLU6(), xc)                                 # not nn.ReLU itself
    assert not norm.fusable2d16(bn, relu, _as_cuda(x[:, :, 0]))                     # not 4-D
    assert not norm.fusable2d16(bn, relu, _as_cuda(x.contiguous(memory_format=torch.channels_last)))   # channels_last
    assert not norm.fusable2d16(bn, relu, _as_cuda(x[:, :, ::2]))                   # strided
    assert not norm.fusable2d16(_bn(4), relu, xc)                                   # channel count
    assert not norm.fusable2d16(bn, relu, _as_cuda(torch.randn(1, 8, 1, 1).half())) # one value per channel in training mode
    assert norm.fusable2d16(bn, relu, _as_cuda(torch.randn(1, 8, 1, 2).half()))
    ev = _bn().eval()
    assert norm.fusable2d16(ev, relu, _as_cuda(torch.randn(1, 8, 1, 1).half()))     # eval mode has no such limit
    assert not norm.fusable2d16(ev, relu, _as_cuda(torch.randn(0, 8, 1, 1).half()))
    nobias = _bn()
    nobias._parameters["bias"] = None
    assert not norm.fusable2d16(nobias, relu, xc)                                   # weight without bias
    torch.set_autocast_enabled(True)                                                # (the flag torch.autocast("cuda") sets; no device needed)
    try:
        assert not norm.fusable2d16(bn, relu, xc)                                   # autocast ...
        spconv.set_mixed_precision(True)
        try:
            assert norm.fusable2d16(bn, relu, xc)                                   # ... unless the 16-bit route was asked for
            assert not norm.fusable2d(bn, relu, xc)
        finally:
            spconv.set_mixed_precision(False)
        assert not norm.fusable2d16(bn, relu, xc)
    finally:
        torch.set_autocast_enabled(False)
    assert norm.fusable2d16(bn, relu, xc)
    saved = norm._ENABLED
    try:
        norm._ENABLED = False
        assert not norm.fusable2d16(bn, relu, xc)
    finally:
        norm._ENABLED = saved


def test_run_maps_on_host_tensors_still_equals_the_modules():
    torch.manual_seed(0)
    make = lambda: nn.Sequential(nn.Conv2d(3, 8, 3, padding=1, bias=False), nn.BatchNorm2d(8, eps=1e-3, momentum=0.01), nn.ReLU(),
                                 nn.Conv2d(8, 4, 1), nn.BatchNorm2d(4))
    for dtype in (torch.float32, torch.bfloat16):
        seq, twin = make().to(dtype), make().to(dtype)
        twin.load_state_dict(seq.state_dict())
        x = torch.randn(2, 3, 5, 7).to(dtype)
        assert torch.equal(norm.run_maps(seq, x), twin(x))
        for a, b in zip(seq.state_dict().values(), twin.state_dict().values()):
            assert torch.equal(a, b)
