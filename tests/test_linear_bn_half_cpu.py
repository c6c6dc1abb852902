"""CPU: the 16-bit Linear + BatchNorm1d (+ReLU) entry points (the 16-bit formats of csrc/linear_bn.hip) exist and are declared, their host-side queries run
without a device, the Python side (pcdet.ops.spconv.linear: fusable16, linear_bn_relu16, run_rows) declines on host tensors, and the
cases file keeps its own conditions: the ReLU kink, the range of z, and a host emulation of the arithmetic contract that stays inside
every derived bound of linear_bn_half_cases.py."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import fv2p_native as nat
import linear_bn_half_cases as cases
from pcdet.ops.spconv import linear

SYMBOLS = ["fv2p_linear_bn_h_supported", "fv2p_linear_bn_h_ws_bytes", "fv2p_linear_bn_h_splits", "fv2p_linear_bn_h_pays",
           "fv2p_linear_bn_forward_h", "fv2p_linear_bn_forward_eval_h", "fv2p_linear_bn_backward_h"]
DTYPES = [torch.float16, torch.bfloat16]
dtype_id = lambda d: str(d).replace("torch.", "")


def test_symbols_are_exported_and_declared():
    raw = ctypes.CDLL(nat.LIB_PATH)
    declared = set(nat.declared_symbols())
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fv2p_ops.h")).read()
    for name in SYMBOLS:
        assert hasattr(raw, name), name
        assert name in declared, name
        assert name + "(" in header, name


def test_host_queries_run_without_a_device():
    ws = lambda n, cin, cout: nat.call("fv2p_linear_bn_h_ws_bytes", n, cin, cout)
    splits = lambda n, cin, cout: nat.call("fv2p_linear_bn_h_splits", n, cin, cout)
    assert ws(1, 1, 1) > 0
    for cin, cout in [(1, 1), (5, 7), (16, 128), (64, 128), (256, 256), (1024, 512)]:
        sizes = [ws(n, cin, cout) for n in (1, 2, 3, 127, 128, 129, 300, 511, 512, 513, 1031, 4096, 49152, 49153, 1 << 20)]
        assert all(s > 0 for s in sizes), (cin, cout, sizes)
        assert sizes == sorted(sizes), (cin, cout, sizes)      # monotone in n
        assert splits(1, cin, cout) == 1
    for n, cin, cout in [(0, 4, 4), (4, 0, 4), (4, 4, 0), (4, 1025, 4), (4, 4, 513)]:   # outside the limits: no workspace, no splits
        assert ws(n, cin, cout) == 0 and splits(n, cin, cout) == 0
        assert nat.call("fv2p_linear_bn_h_supported", n, cin, cout, 1, 1, 1) == 0
    # the weight-gradient chunks of the GPU test: at least three, the last one ragged (chunks are whole 128-row periods)
    n, cin, cout = cases.SPLIT_SHAPE
    s = splits(n, cin, cout)
    assert s >= 3 and n % 128 != 0 and (s - 1) * 128 < n
    assert ws(n, cin, cout) >= s * cin * cout * 8 + cin * cout * 2      # one fp64 [cout][cin] tile per chunk, and w^T in 16 bits
    for dt in (1, 2):
        for wd in (0, dt):
            for pd in (0, dt):
                assert nat.call("fv2p_linear_bn_h_supported", 300, 64, 128, dt, wd, pd) == 1
    for dt, wd, pd in [(0, 0, 0), (3, 0, 0), (-1, 0, 0), (1, 2, 0), (2, 1, 0), (1, 0, 2), (2, 0, 1), (1, 3, 1), (1, 1, 5)]:
        assert nat.call("fv2p_linear_bn_h_supported", 300, 64, 128, dt, wd, pd) == 0, (dt, wd, pd)
    for n, cin, cout in [(49152, 256, 256), (49152, 16, 128), (2, 1, 1), (4, 1025, 4)]:
        for dt in (1, 2):
            assert nat.call("fv2p_linear_bn_h_pays", n, cin, cout, dt) in (0, 1)
    assert nat.call("fv2p_linear_bn_h_pays", 4, 1025, 4, 1) == 0
    assert linear.pays16(4, 1025, 4, torch.float16) is False


def test_python_side_declines_on_host_tensors():
    for dtype in (torch.float32, torch.bfloat16):
        lin, bn, relu = nn.Linear(6, 10, bias=False).to(dtype), nn.BatchNorm1d(10, eps=1e-3, momentum=0.01).to(dtype), nn.ReLU()
        x = torch.randn(5, 6).to(dtype)
        before = {k: v.clone() for k, v in bn.state_dict().items()}
        assert linear.fusable16(lin, bn, relu, x) is False
        assert linear.fusable16(lin, bn, None, x) is False
        assert linear.linear_bn_relu16(lin, bn, x, relu) is None
        assert linear.linear_bn_relu16(lin, bn, x) is None
        assert linear.try_rows(lin, bn, relu, x) is None
        for k, v in bn.state_dict().items():
            assert torch.equal(v, before[k]), k


def test_run_rows_is_the_sequential_on_the_host():
    from fv2p_harness import fv2p_model
    torch.manual_seed(0)
    mk = lambda: nn.Sequential(nn.Linear(6, 10, bias=False), nn.BatchNorm1d(10, eps=1e-3, momentum=0.01), nn.ReLU(),
                               nn.Linear(10, 4, bias=False), nn.BatchNorm1d(4, eps=1e-3, momentum=0.01))
    x = torch.randn(9, 6)
    for run in (linear.run_rows, fv2p_model.run_rows):
        seq, twin = mk(), mk()
        twin.load_state_dict(seq.state_dict())
        assert torch.equal(run(seq, x), twin(x))
        for a, b in zip(seq.state_dict().values(), twin.state_dict().values()):
            assert torch.equal(a, b)


def _forms(dtype):
    """(pdtype, wdtype, relu, affine): uniform T parameters with ReLU + affine; fp32 BatchNorm parameters without; an fp32 master weight."""
    return [(dtype, dtype, True, True), (torch.float32, dtype, False, False), (torch.float32, torch.float32, True, True)]


@pytest.mark.parametrize("n,cin,cout", cases.SHAPES)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_cases_keep_their_conditions_and_the_emulation_stays_inside_every_bound(dtype, n, cin, cout):
    u = cases.UNIT[dtype]
    for tag, (pdtype, wdtype, relu, affine) in enumerate(_forms(dtype)):
        ops = cases.operands(n, cin, cout, dtype, wdtype, pdtype, affine, tag)
        emu, backward = cases.emulate(ops, dtype, pdtype, wdtype, relu)
        # range: no |z| above 8, float16 cannot overflow
        zr, e_z = cases.stage_a(ops["x"], ops["wt"])
        assert np.abs(zr).max() <= cases.Z_MAX and np.abs(emu["z"]).max() <= cases.Z_MAX, np.abs(zr).max()
        # stage A
        assert cases.within(emu["z"], zr, e_z, u).max() <= 1.0
        # stage B on the host-rounded z; the kink: at most 1e-4 of the elements
        b = cases.stage_b(emu["z"], ops["gamma"], ops["beta"], relu, ops["dy"])
        assert b["kink"] <= cases.KINK_FRACTION * n * cout, (b["kink"], n * cout)
        got = backward(b["dy"])
        up = cases.UNIT[pdtype]
        assert (np.abs(emu["mean"] - b["mean"]) <= b["e_mean"]).all()
        assert (np.abs(emu["invstd"] - b["invstd"]) <= b["e_invstd"]).all()
        assert cases.within(emu["y"], b["y"], b["e"], u).max() <= 1.0
        assert cases.within(got["dgamma"], b["dgamma"], b["e_dgamma"], up).max() <= 1.0
        assert cases.within(got["dbeta"], b["dbeta"], 0.0, up).max() <= 1.0
        # stage C
        d_sub = cases.EPS24 if dtype == torch.float16 else 0.0
        assert (np.abs(got["du"] - b["du"]) <= u * (np.abs(b["du"]) + b["e_du"]) + b["e_du"] + d_sub).all()
        dx, e_dx, dw, e_dw = cases.stage_c(b["du"], b["e_du"], ops["x"], ops["wt"], dtype)
        assert cases.within(got["dx"], dx, e_dx, u).max() <= 1.0
        assert cases.within(got["dw"], dw, e_dw, cases.UNIT[wdtype]).max() <= 1.0


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_eval_mode_emulation_stays_inside_the_bounds(dtype):
    u = cases.UNIT[dtype]
    for n, cin, cout in cases.EVAL_SHAPES:
        ops = cases.operands(n, cin, cout, dtype, dtype, dtype, True, 7)
        emu, backward = cases.emulate(ops, dtype, dtype, dtype, True, batch_stats=False)
        b = cases.stage_b(emu["z"], ops["gamma"], ops["beta"], True, ops["dy"], batch_stats=False, rm=ops["rm"], rv=ops["rv"])
        assert b["kink"] <= cases.KINK_FRACTION * n * cout
        got = backward(b["dy"])
        assert cases.within(emu["y"], b["y"], b["e"], u).max() <= 1.0
        dx, e_dx, dw, e_dw = cases.stage_c(b["du"], b["e_du"], ops["x"], ops["wt"], dtype)
        assert cases.within(got["dx"], dx, e_dx, u).max() <= 1.0
        assert cases.within(got["dw"], dw, e_dw, u).max() <= 1.0
        assert cases.within(got["dgamma"], b["dgamma"], b["e_dgamma"], u).max() <= 1.0
        assert cases.within(got["dbeta"], b["dbeta"], 0.0, u).max() <= 1.0
