"""CPU: the mixed-precision sparse conv entry points (fp32 master weights beside 16-bit rows) exist in header and library, and the
process-wide switch `spconv.set_mixed_precision` is off by default, round-trips and leaves the strict dtype rule in place when off."""
import ctypes

import pytest
import torch

import fv2p_native as nat
import pcdet.ops.spconv as spconv
from pcdet.ops.spconv import ops

NEW_SYMBOLS = ["fv2p_sparse_conv_rows_hw32", "fv2p_sparse_conv_wgrad_hw32"]


def test_the_mixed_precision_entry_points_are_declared_and_exported():
    declared = nat.declared_symbols()
    raw = ctypes.CDLL(nat.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, name + " is not declared in include/fv2p_ops.h"
        assert hasattr(raw, name), name + " is not exported by libfv2p_ops.so"
    # the arguments of the uniform 16-bit entry points, in the same order
    for name, sibling in zip(NEW_SYMBOLS, ("fv2p_sparse_conv_rows_h", "fv2p_sparse_conv_wgrad_h")):
        assert [k for k, _, _ in declared[name].params] == [k for k, _, _ in declared[sibling].params]


def test_the_switch_is_off_by_default_round_trips_and_is_restored():
    assert spconv.mixed_precision() is False
    try:
        spconv.set_mixed_precision(True)
        assert spconv.mixed_precision() is True and ops.mixed_precision() is True
        spconv.set_mixed_precision(0)
        assert spconv.mixed_precision() is False
        spconv.set_mixed_precision(1)
        assert spconv.mixed_precision() is True
    finally:
        spconv.set_mixed_precision(False)
    assert spconv.mixed_precision() is False
    assert "set_mixed_precision" in spconv.__all__ and "mixed_precision" in spconv.__all__


def test_the_cached_16_bit_copy_is_keyed_on_the_parameter_version():
    conv = spconv.SubMConv3d(16, 16, 3, padding=1, bias=False)
    a = conv._weight16(torch.bfloat16)
    assert a.dtype == torch.bfloat16 and not a.requires_grad and conv._weight16(torch.bfloat16) is a
    assert conv._weight16(torch.float16) is not a                       # one copy at a time, of the dtype asked for
    with torch.no_grad():
        conv.weight.mul_(2.0)                                           # what an optimiser step does: the version counter moves
    b = conv._weight16(torch.bfloat16)
    assert b is not a and torch.equal(b, conv.weight.detach().to(torch.bfloat16))
    assert "_fv2p_w16" not in conv.state_dict() and len(list(conv.parameters())) == 1
    assert ops.cached_copy_pays(16, 16, None) and not ops.cached_copy_pays(4, 16, None) and not ops.cached_copy_pays(16, 16, conv.weight)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=lambda d: str(d).replace("torch.", ""))
def test_with_the_switch_off_a_mix_of_dtypes_still_raises(dtype):
    assert not spconv.mixed_precision()
    feats, w = torch.zeros(2, 4, dtype=dtype), torch.zeros(27, 4, 4)
    with pytest.raises(TypeError, match="one dtype"):
        ops._conv_dtype(feats, w, None)
    assert not ops.is_mixed(feats, w)
    try:
        spconv.set_mixed_precision(True)
        assert ops.is_mixed(feats, w) and ops.is_mixed(feats, w, torch.zeros(4))
        assert not ops.is_mixed(feats, w.to(dtype)) and not ops.is_mixed(feats.float(), w) and not ops.is_mixed(feats, w, torch.zeros(4, dtype=dtype))
        with pytest.raises(TypeError, match="one dtype"):   # the strict rule itself does not move with the switch
            ops._conv_dtype(feats, w, None)
    finally:
        spconv.set_mixed_precision(False)
