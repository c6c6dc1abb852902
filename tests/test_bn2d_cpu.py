"""CPU: the BatchNorm2d (+ReLU) entry points exist and are declared, the workspace query is monotone, and the Python wrapper declines
(returns None, so the caller runs torch's modules) in every situation it does not cover - checked on host tensors, where it must decline
every time, with a stand-in for `x.is_cuda` where the condition under test is a later one."""
import ctypes
import os

import torch
import torch.nn as nn

import fv2p_native as nat
from pcdet.ops.spconv import norm

SYMBOLS = ["fv2p_batchnorm2d_ws_bytes", "fv2p_batchnorm2d_forward", "fv2p_batchnorm2d_apply", "fv2p_batchnorm2d_backward"]


def test_symbols_are_exported_and_declared():
    raw = ctypes.CDLL(nat.LIB_PATH)
    declared = set(nat.declared_symbols())
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fv2p_ops.h")).read()
    for name in SYMBOLS:
        assert hasattr(raw, name), name
        assert name in declared, name
        assert name + "(" in header, name
    assert nat.lib().fv2p_abi_version() == 1


def test_ws_bytes_is_monotone():
    ws = lambda n, c, hw: nat.call("fv2p_batchnorm2d_ws_bytes", n, c, hw)
    C = norm.BN2D_CHUNK
    base = ws(1, 1, 1)
    assert base > 0
    for n, c, hw in [(1, 1, 1), (2, 5, 35), (3, 128, 200 * 176), (3, 256, 100 * 88)]:
        here = ws(n, c, hw)
        assert ws(n + 1, c, hw) >= here and ws(n, c + 1, hw) >= here and ws(n, c, hw + 1) >= here
        assert ws(4 * n, c, hw) >= here and ws(n, 4 * c, hw) >= here and ws(n, c, 4 * hw + C) >= here
    # one pair of doubles per (sample, channel, chunk): the size steps exactly where a plane needs one more chunk
    assert ws(64, 64, C) == ws(64, 64, 1) < ws(64, 64, C + 1) == ws(64, 64, 2 * C) < ws(64, 64, 2 * C + 1)
    assert ws(3, 256, 200 * 176) >= 3 * 256 * 9 * 16
    assert ws(0, 1, 1) == 0 and ws(1, 0, 1) == 0 and ws(1, 1, 0) == 0


def test_argument_errors_come_back_as_codes():
    lib = nat.lib()
    assert lib.fv2p_batchnorm2d_forward(None, 1, 1, 4, 1e-3, 0.1, None, None, 1, None, None, None, None, None, None, None, 0, None) < 0
    assert "null" in nat.last_error()
    assert lib.fv2p_batchnorm2d_backward(None, None, 0, 1, 4, None, None, None, None, 1, 1, None, None, None, None, 0, None) < 0
    assert "batchnorm2d_backward" in nat.last_error()
    assert lib.fv2p_batchnorm2d_apply(None, 1, 0, 4, None, None, None, None, 1, None, None) < 0


class _AsCuda(torch.Tensor):
    """A host tensor that answers is_cuda = True: lets the wrapper's later conditions be reached without a GPU."""

    @property
    def is_cuda(self):
        return True


def _as_cuda(t):
    return t.as_subclass(_AsCuda)


def test_wrapper_declines_every_uncovered_case_on_host_tensors():
    bn, relu = nn.BatchNorm2d(8), nn.ReLU()
    x = torch.randn(2, 8, 4, 4)
    assert norm.batch_norm2d_relu(bn, x, relu) is None                      # a host tensor
    xc = _as_cuda(x)
    assert norm.fusable2d(bn, relu, xc)                                      # the stand-in reaches the end of the conditions ...
    assert not norm.fusable2d(bn, relu, x)                                   # ... which a real host tensor does not

    class MyBn(nn.BatchNorm2d):
        pass
    assert not norm.fusable2d(MyBn(8), relu, xc)                             # type(bn) is not nn.BatchNorm2d
    assert not norm.fusable2d(nn.BatchNorm1d(8), relu, xc)
    assert not norm.fusable2d(nn.SyncBatchNorm(8), relu, xc)
    hooked = nn.BatchNorm2d(8)
    hooked.register_forward_hook(lambda m, i, o: None)
    assert not norm.fusable2d(hooked, relu, xc)                              # hooks
    pre = nn.BatchNorm2d(8)
    pre.register_forward_pre_hook(lambda m, i: None)
    assert not norm.fusable2d(pre, relu, xc)
    patched = nn.BatchNorm2d(8)
    patched.forward = lambda t: t
    assert not norm.fusable2d(patched, relu, xc)                             # forward replaced on the instance
    hrelu = nn.ReLU()
    hrelu.register_forward_hook(lambda m, i, o: None)
    assert not norm.fusable2d(bn, hrelu, xc)
    prelu = nn.ReLU()
    prelu.forward = lambda t: t
    assert not norm.fusable2d(bn, prelu, xc)
    assert not norm.fusable2d(bn, nn.ReLU6(), xc)                            # not nn.ReLU itself
    assert not norm.fusable2d(bn, relu, _as_cuda(x.double()))                # dtype
    assert not norm.fusable2d(bn, relu, _as_cuda(x.half()))
    assert not norm.fusable2d(bn, relu, _as_cuda(x[:, :, 0]))                # not 4-D
    assert not norm.fusable2d(bn, relu, _as_cuda(x.contiguous(memory_format=torch.channels_last)))   # channels_last
    assert not norm.fusable2d(bn, relu, _as_cuda(x[:, :, ::2]))              # strided
    assert not norm.fusable2d(nn.BatchNorm2d(4), relu, xc)                   # channel count
    assert not norm.fusable2d(bn, relu, _as_cuda(torch.randn(1, 8, 1, 1)))   # n * hw = 1 in training mode
    assert norm.fusable2d(bn, relu, _as_cuda(torch.randn(1, 8, 1, 2)))
    ev = nn.BatchNorm2d(8).eval()
    assert norm.fusable2d(ev, relu, _as_cuda(torch.randn(1, 8, 1, 1)))       # eval mode has no such limit
    assert not norm.fusable2d(ev, relu, _as_cuda(torch.randn(0, 8, 1, 1)))
    torch.set_autocast_enabled(True)                                         # (the flag torch.autocast("cuda") sets; no device needed)
    try:
        assert not norm.fusable2d(bn, relu, xc)                              # autocast
    finally:
        torch.set_autocast_enabled(False)
    assert norm.fusable2d(bn, relu, xc)
    assert not norm.fusable2d(nn.BatchNorm2d(8).double(), relu, xc)          # parameters not fp32
    half_stats = nn.BatchNorm2d(8)
    half_stats.running_var = half_stats.running_var.half()
    assert not norm.fusable2d(half_stats, relu, xc)
    meta = nn.BatchNorm2d(8, device="meta")
    assert not norm.fusable2d(meta, relu, xc)                                # parameters on another device than x
    saved = norm._ENABLED
    try:
        norm._ENABLED = False
        assert not norm.fusable2d(bn, relu, xc)
    finally:
        norm._ENABLED = saved


def test_run_maps_falls_back_to_the_modules_on_the_host():
    torch.manual_seed(0)
    seq = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1, bias=False), nn.BatchNorm2d(8, eps=1e-3, momentum=0.01), nn.ReLU(),
                        nn.Conv2d(8, 4, 1), nn.BatchNorm2d(4))
    twin = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1, bias=False), nn.BatchNorm2d(8, eps=1e-3, momentum=0.01), nn.ReLU(),
                         nn.Conv2d(8, 4, 1), nn.BatchNorm2d(4))
    twin.load_state_dict(seq.state_dict())
    x = torch.randn(2, 3, 5, 7)
    assert torch.equal(norm.run_maps(seq, x), twin(x))
    for a, b in zip(seq.state_dict().values(), twin.state_dict().values()):
        assert torch.equal(a, b)


def test_reference_call_structure_switches_the_op_off():
    from fv2p_harness import refstyle
    inside = None
    before = norm.fusable2d
    with refstyle.reference_call_structure():
        inside = norm.fusable2d(nn.BatchNorm2d(8), nn.ReLU(), _as_cuda(torch.randn(2, 8, 4, 4)))
    assert inside is False and norm.fusable2d is before
