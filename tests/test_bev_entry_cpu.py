"""CPU: the torch statement of pcdet.ops.spconv.bev_entry (gather -> matmul -> index_add over 9 * D offsets) against float64 F.conv2d of
the densified input, forward, dX at the active rows and dW, on the cases of tests/bev_entry_cases.py that need no GPU.  The statement runs
in float64 here, so it must agree to rounding of float64 sums taken in another order (1e-10 on values of order 1)."""
import pytest
import torch

import pcdet.ops.spconv as spconv
from pcdet.ops.spconv import bev_entry as BE

from bev_entry_cases import case

CASES = ["corners", "mixed", "empty_sample", "n0", "full", "d1", "d3", "odd_channels"]
TOL = 1e-10


@pytest.mark.parametrize("name", CASES)
def test_torch_statement_matches_float64_conv2d(name):
    c = case(name)
    f = c["features"].double().requires_grad_(True)
    w = c["weight"].double().requires_grad_(True)
    y = BE.bev_entry_conv_torch(f, c["indices"], c["geom"], w)
    assert y.shape == c["refs"]["y"].shape and y.is_contiguous()
    dx, dw = torch.autograd.grad(y, [f, w], c["grad"].double())
    for n, got in (("y", y.detach()), ("dx", dx), ("dw", dw)):
        err = (got - c["refs"][n]).abs().max().item() if got.numel() else 0.0
        print(f"case {name} {n}: error {err:.3e}")
        assert got.shape == c["refs"][n].shape and err <= TOL, (n, err)


def test_cpu_tensors_take_the_torch_statement():
    c = case("mixed")
    b, d, h, w = c["geom"]
    sp = spconv.SparseConvTensor(c["features"], c["indices"], [d, h, w], b)
    assert BE.route(sp, c["weight"]) == "torch"
    before = BE.ROUTES["torch"]
    y = spconv.bev_entry_conv(sp, c["weight"])
    assert BE.ROUTES["torch"] == before + 1
    assert torch.equal(y, BE.bev_entry_conv_torch(c["features"], c["indices"], c["geom"], c["weight"]))
    assert (y.double() - c["refs"]["y"]).abs().max().item() < 1e-4


def test_weight_repack_is_the_dense_view_order():
    """Channel c * D + z of the Conv2d weight is (c, z) of dense().view(B, C * D, H, W): offset k = z * 9 + ky * 3 + kx reads it."""
    cout, c, d = 3, 4, 2
    w = torch.arange(cout * c * d * 9, dtype=torch.float32).view(cout, c * d, 3, 3)
    wk = BE.repack_weight(w, d)
    assert wk.shape == (9 * d, c, cout)
    for z in range(d):
        for ky in range(3):
            for kx in range(3):
                assert torch.equal(wk[z * 9 + ky * 3 + kx], w[:, z::d, ky, kx].t())
