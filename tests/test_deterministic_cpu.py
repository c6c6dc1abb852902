"""Deterministic mode without a GPU: the switch, the new C-ABI entry points, and which entry point every wrapper reaches with the mode off
(the existing one, unchanged) and on (its fixed-order *_gather form), and that float16 / bfloat16 tensors reach the *_h one either way.
The library calls are recorded, not executed."""
import contextlib
import types

import pytest
import torch

import fv2p_native as _nat
import pcdet.ops as ops
from pcdet.ops import _glue as G

NEW = ["fv2p_scatter_add", "fv2p_group_points_batch_grad_gather", "fv2p_gather_points_grad_gather", "fv2p_group_points_stack_grad_gather",
       "fv2p_three_interpolate_batch_grad_gather", "fv2p_bev_interp_bwd_gather", "fv2p_roiaware_pool3d_bwd_gather",
       "fv2p_deform_psroi_pool_backward_gather", "fv2p_sa_grid_bwd_gather"]


def test_new_entry_points_are_declared_exported_and_sized():
    declared = _nat.declared_symbols()
    lib = _nat.lib()
    for name in NEW:
        assert name in declared, name
        getattr(lib, name)
    ws = {"fv2p_scatter_add_ws_bytes": (1000, 16), "fv2p_group_points_batch_grad_ws_bytes": (2, 16, 100, 64, 16),
          "fv2p_gather_points_grad_ws_bytes": (2, 16, 100, 64), "fv2p_group_points_stack_grad_ws_bytes": (64, 16, 16),
          "fv2p_three_interpolate_batch_grad_ws_bytes": (2, 16, 100, 50), "fv2p_bev_interp_bwd_ws_bytes": (2, 16, 20, 20, 1, 100),
          "fv2p_roiaware_pool3d_bwd_ws_bytes": (4, 6, 6, 6, 16, 128, 1), "fv2p_deform_psroi_pool_backward_ws_bytes": (8, 16, 7, 4),
          "fv2p_sa_grid_bwd_gather_ws_bytes": (8, 216, 16)}
    for name, args in ws.items():
        assert getattr(lib, name)(*args) > 0, name
    # the workspace grows with the entries (a caller sizing for the largest call can reuse it)
    assert lib.fv2p_scatter_add_ws_bytes(10 ** 6, 16) > lib.fv2p_scatter_add_ws_bytes(10 ** 3, 16)


def test_switch_is_process_wide_and_off_by_default():
    assert ops.is_deterministic() is False
    ops.set_deterministic(True)
    try:
        assert ops.is_deterministic() and _nat.deterministic()
        ext = _nat.torch_ext()
        if ext is not None:
            assert ext.deterministic()
    finally:
        ops.set_deterministic(False)
    assert not ops.is_deterministic()
    ext = _nat.torch_ext()
    if ext is not None:
        assert not ext.deterministic()


def test_switch_is_independent_of_torch_deterministic_algorithms():
    saved = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        assert not ops.is_deterministic()
    finally:
        torch.use_deterministic_algorithms(saved)


@pytest.fixture
def recorded(monkeypatch):
    """Every library call answered by a recorder: the names reached, in order."""
    names = []

    def call(name, *args):
        names.append(name)
        return 0
    monkeypatch.setattr(_nat, "call", call)
    monkeypatch.setattr(G, "run", lambda name, *a: names.append(name))
    monkeypatch.setattr(G, "scratch", lambda *a: torch.empty(16, dtype=torch.uint8))
    monkeypatch.setattr(_nat, "workspace", lambda nbytes, dev: torch.empty(16, dtype=torch.uint8))
    monkeypatch.setattr(_nat, "stream", lambda: 0)
    monkeypatch.setattr(_nat, "require_cuda", lambda *a: None)
    monkeypatch.setattr(_nat, "device_guard", lambda dev: contextlib.nullcontext())
    yield names
    ops.set_deterministic(False)


def _wrappers():
    """(existing entry point, its fixed-order form, a call of the wrapper that reaches it) for every site."""
    from pcdet.ops.pointnet2.pointnet2_batch import pointnet2_utils as pb, pointnet2_batch_cuda as pbc, fused
    from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils as ps, pointnet2_stack_cuda as psc
    from pcdet.ops.roiaware_pool3d import roiaware_pool3d_utils as ru, roiaware_pool3d_cuda as rc
    from pcdet.models.backbones_3d.pfe import bev_grid_pooling as bev
    from pcdet.ops.DeformableConvolutionV2PyTorch import DCN
    f, i = torch.zeros(2, 3, 4), torch.zeros(2, 3, 4, dtype=torch.int32)
    cnt = torch.tensor([2], dtype=torch.int32)
    sa = {"t": (torch.zeros(1, 5, 64), torch.zeros(1, 2, 64), torch.zeros(1, 2, 16, dtype=torch.int32), torch.zeros(64, 64),
                torch.zeros(1, 2, 64, dtype=torch.uint8)), "dims": (1, 5, 2, 16, 64)}
    bev_ctx = types.SimpleNamespace(saved_tensors=(torch.zeros(1, 4), torch.zeros(1, 4)), geom=(1, 3, 5, 6, True))
    rois = torch.tensor([[0.0, 1, 1, 4, 4]])
    return [
        ("fv2p_group_points_batch_grad", lambda: pb._group_grad({"shape": (2, 3, 4, 5, 6), "idx": i}, torch.zeros(2, 3, 5, 6))),
        ("fv2p_gather_points_grad", lambda: pb._gather_grad({"shape": (2, 3, 4, 5), "idx": i}, torch.zeros(2, 3, 5))),
        ("fv2p_three_interpolate_batch_grad",
         lambda: pb._interp_grad({"shape": (2, 3, 4, 5), "idx": i, "weight": f}, torch.zeros(2, 3, 5))),
        ("fv2p_group_points_batch_grad", lambda: pbc.group_points_grad_wrapper(2, 3, 4, 5, 6, torch.zeros(2, 3, 5, 6), i, torch.zeros(2, 3, 4))),
        ("fv2p_gather_points_grad", lambda: pbc.gather_points_grad_wrapper(2, 3, 4, 5, torch.zeros(2, 3, 5), i, torch.zeros(2, 3, 4))),
        ("fv2p_three_interpolate_batch_grad",
         lambda: pbc.three_interpolate_grad_wrapper(2, 3, 5, 4, torch.zeros(2, 3, 5), i, f, torch.zeros(2, 3, 4))),
        ("fv2p_group_points_stack_grad",
         lambda: ps._group_grad({"dims": (1, 2, 3, 4, 5), "idx": i, "ic": cnt, "fc": cnt}, torch.zeros(2, 3, 5))),
        ("fv2p_three_interpolate_stack_grad", lambda: ps._interp_grad({"rows": 4, "idx": i, "weight": f}, torch.zeros(100, 3))),
        ("fv2p_group_points_stack_grad",
         lambda: psc.group_points_grad_wrapper(1, 2, 3, 4, 5, torch.zeros(2, 3, 5), i, cnt, cnt, torch.zeros(4, 3))),
        ("fv2p_three_interpolate_stack_grad",
         lambda: psc.three_interpolate_grad_wrapper(torch.zeros(100, 3), torch.zeros(100, 3, dtype=torch.int32), torch.zeros(100, 3),
                                                    torch.zeros(4, 3))),
        ("fv2p_roiaware_pool3d_bwd",
         lambda: ru._pool_grad({"dims": (1, 2, 2, 2, 3, 7, 4), "members": i, "argmax": i, "code": 1}, torch.zeros(1, 2, 2, 2, 3))),
        ("fv2p_roiaware_pool3d_bwd",
         lambda: rc.backward(torch.zeros(1, 2, 2, 2, 4, dtype=torch.int32), torch.zeros(1, 2, 2, 2, 3, dtype=torch.int32),
                             torch.zeros(1, 2, 2, 2, 3), torch.zeros(7, 3), 0)),
        ("fv2p_sa_grid_bwd", lambda: fused._bwd(sa, torch.zeros(1, 2, 64))),
        ("fv2p_bev_interp_bwd", lambda: bev._BevInterp.backward(bev_ctx, torch.zeros(1, 4, 3))),
        ("fv2p_deform_psroi_pool_backward",
         lambda: DCN.deform_psroi_pooling_backward(torch.zeros(1, 3, 2, 2), torch.zeros(1, 3, 8, 8), rois, torch.zeros(1, 2, 2, 2),
                                                   torch.zeros(1, 3, 2, 2), False, 1.0, 3, 1, 2, 2, 2, 0.1)),
    ]


@pytest.mark.parametrize("k", range(15))
def test_each_wrapper_reaches_the_existing_entry_point_when_off_and_the_fixed_order_one_when_on(recorded, k):
    name, fn = _wrappers()[k]
    fn()
    assert recorded == [name], recorded
    recorded.clear()
    ops.set_deterministic(True)
    fn()
    assert recorded == [name + "_gather"], recorded


def test_stack_interpolation_keeps_its_size_rule_when_off(recorded):
    """Off: below 8192 queries the scatter form, from 8192 on the gather form (as before); on: the gather form at every size."""
    from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils as ps
    i = torch.zeros(1, 3, dtype=torch.int32)
    for n in (100, ps.GATHER_GRAD_MIN_QUERIES):
        ps._interp_grad({"rows": 4, "idx": i, "weight": torch.zeros(1, 3)}, torch.zeros(n, 3))
    assert recorded == ["fv2p_three_interpolate_stack_grad", "fv2p_three_interpolate_stack_grad_gather"]


def _half_sites(dt, queries=100):
    """(existing entry point, a call on float16 / bfloat16 host tensors) for the ten pointnet2 gradient sites: the first ten of _wrappers()."""
    from pcdet.ops.pointnet2.pointnet2_batch import pointnet2_utils as pb, pointnet2_batch_cuda as pbc
    from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils as ps, pointnet2_stack_cuda as psc
    z = lambda *shape: torch.zeros(*shape, dtype=dt)
    f, i = torch.zeros(2, 3, 4), torch.zeros(2, 3, 4, dtype=torch.int32)
    cnt = torch.tensor([2], dtype=torch.int32)
    qi, qw = torch.zeros(queries, 3, dtype=torch.int32), torch.zeros(queries, 3)
    return [
        ("fv2p_group_points_batch_grad", lambda: pb._group_grad({"shape": (2, 3, 4, 5, 6), "idx": i}, z(2, 3, 5, 6))),
        ("fv2p_gather_points_grad", lambda: pb._gather_grad({"shape": (2, 3, 4, 5), "idx": i}, z(2, 3, 5))),
        ("fv2p_three_interpolate_batch_grad", lambda: pb._interp_grad({"shape": (2, 3, 4, 5), "idx": i, "weight": f}, z(2, 3, 5))),
        ("fv2p_group_points_batch_grad", lambda: pbc.group_points_grad_wrapper(2, 3, 4, 5, 6, z(2, 3, 5, 6), i, z(2, 3, 4))),
        ("fv2p_gather_points_grad", lambda: pbc.gather_points_grad_wrapper(2, 3, 4, 5, z(2, 3, 5), i, z(2, 3, 4))),
        ("fv2p_three_interpolate_batch_grad", lambda: pbc.three_interpolate_grad_wrapper(2, 3, 5, 4, z(2, 3, 5), i, f, z(2, 3, 4))),
        ("fv2p_group_points_stack_grad", lambda: ps._group_grad({"dims": (1, 2, 3, 4, 5), "idx": i, "ic": cnt, "fc": cnt}, z(2, 3, 5))),
        ("fv2p_three_interpolate_stack_grad", lambda: ps._interp_grad({"rows": 4, "idx": qi, "weight": qw}, z(queries, 3))),
        ("fv2p_group_points_stack_grad", lambda: psc.group_points_grad_wrapper(1, 2, 3, 4, 5, z(2, 3, 5), i, cnt, cnt, z(4, 3))),
        ("fv2p_three_interpolate_stack_grad", lambda: psc.three_interpolate_grad_wrapper(z(queries, 3), qi, qw, z(4, 3))),
    ]


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["float16", "bfloat16"])
@pytest.mark.parametrize("k", range(10))
def test_each_pointnet2_gradient_site_reaches_the_16_bit_entry_point_whatever_the_switch_says(recorded, k, dt):
    from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils as ps
    sizes = (100, ps.GATHER_GRAD_MIN_QUERIES) if k in (7, 9) else (100,)   # the stack interpolation: below and at its size rule
    for queries in sizes:
        name, fn = _half_sites(dt, queries)[k]
        for on in (False, True):
            recorded.clear()
            ops.set_deterministic(on)
            fn()
            assert recorded == [name + "_h"], (queries, on, recorded)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["float16", "bfloat16"])
def test_stack_ext_wrappers_send_16_bit_tensors_to_the_16_bit_entry_points_and_refuse_mixed_dtypes(recorded, dt):
    from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_stack_cuda as psc
    z = lambda *shape: torch.zeros(*shape, dtype=dt)
    i, cnt = torch.zeros(2, 5, dtype=torch.int32), torch.tensor([2], dtype=torch.int32)
    qi, qw = torch.zeros(6, 3, dtype=torch.int32), torch.zeros(6, 3)
    assert psc.group_points_wrapper(1, 2, 3, 5, z(4, 3), cnt, i, cnt, z(2, 3, 5)) == 1
    assert psc.three_interpolate_wrapper(z(4, 3), qi, qw, z(6, 3)) == 1
    assert recorded == ["fv2p_group_points_stack_h", "fv2p_three_interpolate_stack_h"], recorded
    recorded.clear()
    for call in (lambda: psc.group_points_wrapper(1, 2, 3, 5, z(4, 3), cnt, i, cnt, torch.zeros(2, 3, 5)),
                 lambda: psc.group_points_grad_wrapper(1, 2, 3, 4, 5, z(2, 3, 5), i, cnt, cnt, torch.zeros(4, 3)),
                 lambda: psc.three_interpolate_wrapper(torch.zeros(4, 3), qi, qw, z(6, 3)),
                 lambda: psc.three_interpolate_grad_wrapper(z(6, 3), qi, qw, torch.zeros(4, 3))):
        with pytest.raises(TypeError, match="one dtype"):
            call()
    assert recorded == []
