"""Host: the C ABI of the 16-bit deformable-convolution backward (csrc/dcn_bwd_h.hip) - symbols, the geometry predicate, the workspace
query - and the conditions of the exact cases (dcn_bwd_half_cases.exact_case asserts them).  No GPU."""
import pytest

import dcn_bwd_half_cases as bcases
import dcn_half_cases as cases
import fv2p_native as nat

# the shapes of profiles/dcn_half.txt: (B, Cin = Cout, H, W, deformable groups)
PROFILE_SHAPES = [(4, 256, 200, 176, 4), (4, 128, 200, 176, 1), (4, 256, 100, 88, 4), (4, 256, 50, 44, 4)]   # the MGAF head first


def test_the_three_symbols_exist():
    declared = nat.declared_symbols()
    for name in ("fv2p_dcn_backward_h", "fv2p_dcn_backward_h_supported", "fv2p_dcn_backward_h_ws_bytes"):
        assert name in declared, name
        assert getattr(nat.lib(), name) is not None
    assert len(declared["fv2p_dcn_backward_h"].params) == 5 + 16 + 9


@pytest.mark.parametrize("cin,cout,dg,want", [
    (64, 64, 1, 1), (256, 256, 4, 1), (48, 16, 3, 1), (96, 24, 2, 1), (32, 8, 1, 1), (128, 200, 4, 1),
    (64, 264, 1, 0),      # more than 256 output channels
    (64, 20, 1, 0),       # output channels no multiple of 8 (the caller pads)
    (16, 24, 2, 0),       # 8 channels per deformable group
    (64, 64, 3, 0),       # groups do not divide the channels
    (64, 64, 0, 0), (0, 64, 1, 0), (64, 0, 1, 0),
])
def test_the_supported_truth_table(cin, cout, dg, want):
    assert nat.lib().fv2p_dcn_backward_h_supported(cin, cout, dg) == want
    if want:
        assert nat.lib().fv2p_dcn_forward_h_supported(cin, cout, dg) == 1


@pytest.mark.parametrize("shape", PROFILE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_workspace_is_positive_and_below_the_fp32_backwards(shape):
    B, C, H, W, dg = shape
    half = nat.lib().fv2p_dcn_backward_h_ws_bytes(B, H, W, H, W, C, C, 3, 3, dg)
    full = nat.lib().fv2p_dcn_backward_ws_bytes(B, H, W, H, W, C, C, 3, 3, dg)
    assert 0 < half < full, (half, full)
    # the column gradients dominate both: two bytes an element against four
    assert half >= B * H * W * 9 * C * 2


@pytest.mark.parametrize("family,g", cases.EXACT, ids=lambda v: v if isinstance(v, str) else cases.geom_id(v))
def test_the_exact_cases_meet_their_conditions(family, g):
    case = bcases.exact_case(family, g)
    assert case["dcol_top"] <= 22.0 and case["top"] <= 137.0
    assert float(case["dy"].abs().mean()) < 0.25 and set(case["dy"].unique().tolist()) <= {-1.0, 0.0, 1.0}
