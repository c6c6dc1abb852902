"""CPU: the Linear + BatchNorm1d (+ReLU) entry points (csrc/linear_bn.hip) exist and are declared, their three host-side queries run
without a device, and the Python side (pcdet.ops.spconv.linear) declines on host tensors - so the caller runs torch's modules."""
import ctypes
import os

import torch
import torch.nn as nn

import fv2p_native as nat
from pcdet.ops.spconv import linear

SYMBOLS = ["fv2p_linear_bn_ws_bytes", "fv2p_linear_bn_splits", "fv2p_linear_bn_pays", "fv2p_linear_bn_forward",
           "fv2p_linear_bn_forward_eval", "fv2p_linear_bn_backward"]
SPLIT_ROWS = 300          # the row count tests/test_linear_bn_gpu.py uses for the weight-gradient splits at (., 64, 128)


def test_symbols_are_exported_and_declared():
    raw = ctypes.CDLL(nat.LIB_PATH)
    declared = set(nat.declared_symbols())
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fv2p_ops.h")).read()
    for name in SYMBOLS:
        assert hasattr(raw, name), name
        assert name in declared, name
        assert name + "(" in header, name


def test_host_queries_run_without_a_device():
    ws = lambda n, cin, cout: nat.call("fv2p_linear_bn_ws_bytes", n, cin, cout)
    splits = lambda n, cin, cout: nat.call("fv2p_linear_bn_splits", n, cin, cout)
    assert ws(1, 1, 1) > 0
    for cin, cout in [(1, 1), (5, 7), (16, 128), (64, 128), (256, 256), (1024, 512)]:
        sizes = [ws(n, cin, cout) for n in (1, 2, 3, 127, 128, 129, 300, 511, 512, 513, 1031, 4096, 49152, 49153, 1 << 20)]
        assert all(s > 0 for s in sizes), (cin, cout, sizes)
        assert sizes == sorted(sizes), (cin, cout, sizes)      # never decreases in n
        assert splits(1, cin, cout) == 1
    # outside the limits: no workspace, no splits
    for n, cin, cout in [(0, 4, 4), (4, 0, 4), (4, 4, 0), (4, 1025, 4), (4, 4, 513)]:
        assert ws(n, cin, cout) == 0 and splits(n, cin, cout) == 0
    # the weight-gradient chunks of the GPU test: at least three, the last one ragged (chunks are whole 128-row periods)
    s = splits(SPLIT_ROWS, 64, 128)
    assert s >= 3 and SPLIT_ROWS % 128 != 0 and (s - 1) * 128 < SPLIT_ROWS
    # the workspace holds one fp64 [cout][cin] tile per chunk
    assert ws(SPLIT_ROWS, 64, 128) >= s * 64 * 128 * 8
    for n, cin, cout in [(49152, 256, 256), (49152, 16, 128), (2, 1, 1)]:
        assert nat.call("fv2p_linear_bn_pays", n, cin, cout) in (0, 1)
    assert nat.call("fv2p_linear_bn_pays", 4, 1025, 4) == 0


def test_python_side_declines_on_host_tensors():
    lin, bn, relu = nn.Linear(6, 10, bias=False), nn.BatchNorm1d(10, eps=1e-3, momentum=0.01), nn.ReLU()
    x = torch.randn(5, 6)
    before = {k: v.clone() for k, v in bn.state_dict().items()}
    assert linear.fusable(lin, bn, relu, x) is False
    assert linear.fusable(lin, bn, None, x) is False
    assert linear.linear_bn_relu(lin, bn, x, relu) is None
    assert linear.linear_bn_relu(lin, bn, x) is None
    for k, v in bn.state_dict().items():
        assert torch.equal(v, before[k]), k


def test_run_rows_is_the_sequential_on_the_host():
    torch.manual_seed(0)
    mk = lambda: nn.Sequential(nn.Linear(6, 10, bias=False), nn.BatchNorm1d(10, eps=1e-3, momentum=0.01), nn.ReLU(),
                               nn.Linear(10, 4, bias=False), nn.BatchNorm1d(4, eps=1e-3, momentum=0.01))
    seq, twin = mk(), mk()
    twin.load_state_dict(seq.state_dict())
    x = torch.randn(9, 6)
    assert torch.equal(linear.run_rows(seq, x), twin(x))
    for a, b in zip(seq.state_dict().values(), twin.state_dict().values()):
        assert torch.equal(a, b)
