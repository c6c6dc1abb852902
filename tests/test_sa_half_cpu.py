"""CPU: the 16-bit fused grid set-abstraction (csrc/sa_fused.hip) exists in header and library, sizes its workspace on the host,
rejects bad arguments before anything touches a device, and pcdet.ops.pointnet2.pointnet2_batch.fused reaches it for float16 /
bfloat16 rows - whatever the deterministic switch says - while float32 rows keep their three entry points.  The library calls are
recorded, not executed."""
import contextlib

import pytest
import torch

import fv2p_native as _nat
import pcdet.ops as ops
from pcdet.ops import _glue as G
from pcdet.ops.pointnet2.pointnet2_batch import fused

import sa_half_cases as cases

NEW = {"fv2p_sa_grid_supported_h": 4, "fv2p_sa_grid_fwd_h": 14, "fv2p_sa_grid_bwd_h_ws_bytes": 3, "fv2p_sa_grid_bwd_h": 19}
EINVAL = -1
P = 4096          # stands for a non-null, aligned device pointer: every call below is rejected before it is looked at


def test_the_four_names_are_declared_and_exported():
    declared = _nat.declared_symbols()
    lib = _nat.lib()
    for name, n in NEW.items():
        assert name in declared, name
        assert len(declared[name].params) == n, name
        getattr(lib, name)
    assert lib.fv2p_abi_version() == 1


def test_workspace_query_is_a_host_function_and_grows_with_its_arguments():
    ws = _nat.lib().fv2p_sa_grid_bwd_h_ws_bytes
    assert ws(8, 216, 16) > 0 and ws(0, 0, 0) > 0
    base = [8, 216, 16]
    for pos in range(3):
        sizes = [ws(*(base[:pos] + [v] + base[pos + 1:])) for v in (1, 2, 16, 32, 100, 1000)]
        assert sizes == sorted(sizes) and sizes[0] < sizes[-1], (pos, sizes)
    # the dh1 rows are staged in 16 bits: at the RoI head's shape the workspace stays below the fp32 fixed-order form's
    assert ws(384, 216, 32) < _nat.lib().fv2p_sa_grid_bwd_gather_ws_bytes(384, 216, 32)
    assert ws(384, 216, 32) >= 384 * 216 * 32 * 64 * 2


def test_supported_h_answers_for_shapes_not_for_a_point_count():
    sup = _nat.lib().fv2p_sa_grid_supported_h
    assert sup(512, 216, 16, 64) == 1 and sup(512, 216, 32, 64) == 1
    assert sup(1000, 17, 16, 64) == 1 and sup(100000, 17, 16, 64) == 1          # no dP tile in LDS: the fp32 backward's n <= 884 is gone
    assert _nat.lib().fv2p_sa_grid_supported(1000, 17, 16, 64) == 0
    for n, m, s, c in [(512, 216, 8, 64), (512, 216, 24, 64), (512, 216, 64, 64), (512, 216, 16, 32), (512, 216, 16, 128), (0, 216, 16, 64),
                       (512, 0, 16, 64)]:
        assert sup(n, m, s, c) == 0, (n, m, s, c)


@pytest.mark.parametrize("what,kw", [("dtype", dict(dtype=0)), ("dtype", dict(dtype=3)), ("wd", dict(wd=2)), ("null pointer", dict(null=True)),
                                     ("64 channels", dict(c=32)), ("64 channels", dict(s=24)), ("64 channels", dict(rois=0)),
                                     ("aligned", dict(ptr=P + 2))],
                         ids=["dtype0", "dtype3", "wd-other-format", "null", "c32", "s24", "rois0", "misaligned"])
def test_bad_arguments_are_rejected_before_any_launch(what, kw):
    lib = _nat.lib()
    dtype, wd, c, s, rois = kw.get("dtype", 1), kw.get("wd", 0), kw.get("c", 64), kw.get("s", 16), kw.get("rois", 2)
    ptr = None if kw.get("null") else kw.get("ptr", P)
    assert lib.fv2p_sa_grid_fwd_h(ptr, P, P, P, wd, rois, 9, 4, s, c, P, None, dtype, None) == EINVAL
    assert what in _nat.last_error(), _nat.last_error()
    assert lib.fv2p_sa_grid_bwd_h(ptr, P, P, P, wd, P, P, rois, 9, 4, s, c, P, P, P, dtype, P, 1 << 40, None) == EINVAL
    assert what in _nat.last_error(), _nat.last_error()


def test_backward_refuses_a_small_workspace_and_too_many_samples():
    lib = _nat.lib()
    assert lib.fv2p_sa_grid_bwd_h(P, P, P, P, 0, P, P, 2, 9, 4, 16, 64, P, P, P, 1, P, 16, None) == -2      # FV2P_EWORKSPACE
    assert "workspace" in _nat.last_error()
    assert lib.fv2p_sa_grid_bwd_h(P, P, P, P, 0, P, P, 65535, 9, 4096, 16, 64, P, P, P, 1, P, 1 << 60, None) == -4   # FV2P_ELIMIT
    assert "too many samples" in _nat.last_error()


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


def _operands(dt, wdt):
    z = lambda *shape, d=dt: torch.zeros(*shape, dtype=d)
    return z(1, 5, 64).requires_grad_(True), z(1, 2, 64), torch.zeros(1, 2, 16, dtype=torch.int32), z(64, 64, d=wdt)


@pytest.mark.parametrize("w32", [False, True], ids=["w16", "w32"])
@pytest.mark.parametrize("dt", cases.DTYPES, ids=cases.dtype_id)
def test_rows_reach_the_entry_points_of_their_dtype(recorded, dt, w32):
    pp, pc, idx, w2 = _operands(dt, torch.float32 if w32 else dt)
    saved = {}
    out = fused._fwd(saved, pp, pc, idx, w2)
    assert recorded == ["fv2p_sa_grid_fwd_h"], recorded
    assert out.dtype == dt and out.shape == (1, 2, 64) and saved["t"][4].dtype == torch.uint8 and saved["dims"] == (1, 5, 2, 16, 64)
    for on in (False, True):
        recorded.clear()
        ops.set_deterministic(on)
        gp, gc, none, gw = fused._bwd(saved, torch.zeros(1, 2, 64, dtype=dt))
        assert recorded == ["fv2p_sa_grid_bwd_h"], (on, recorded)
        assert gp.dtype == dt and gc.dtype == dt and none is None and gw.dtype == w2.dtype
        assert gp.shape == pp.shape and gc.shape == pc.shape and gw.shape == w2.shape
    # ... and float32 rows keep their three entry points, the `saved` keys and the two backward routes
    ops.set_deterministic(False)
    recorded.clear()
    pp, pc, idx, w2 = _operands(torch.float32, torch.float32)
    saved = {}
    out = fused._fwd(saved, pp, pc, idx, w2)
    assert recorded == ["fv2p_sa_grid_fwd"] and out.dtype == torch.float32 and sorted(saved) == ["dims", "t"]
    recorded.clear()
    fused._bwd(saved, torch.zeros(1, 2, 64))
    ops.set_deterministic(True)
    fused._bwd(saved, torch.zeros(1, 2, 64))
    assert recorded == ["fv2p_sa_grid_bwd", "fv2p_sa_grid_bwd_gather"], recorded


@pytest.mark.parametrize("dt", cases.DTYPES, ids=cases.dtype_id)
def test_mixed_row_dtypes_raise_and_nothing_is_recorded(recorded, dt):
    other = torch.bfloat16 if dt == torch.float16 else torch.float16
    pp, pc, idx, w2 = _operands(dt, dt)
    for bad in (torch.float32, other):
        with pytest.raises(TypeError, match="one dtype"):
            fused._fwd({}, pp, pc.to(bad), idx, w2)
        with pytest.raises(TypeError, match="one dtype"):
            fused._fwd({}, pp.detach().to(bad), pc, idx, w2)
    with pytest.raises(TypeError, match="float32"):
        fused._fwd({}, pp, pc, idx, w2.to(other))                    # the weight: the rows' dtype or float32, nothing else
    assert recorded == []
    saved = {}
    fused._fwd(saved, pp, pc, idx, w2)
    recorded.clear()
    for bad in (torch.float32, other):
        with pytest.raises(TypeError, match="one dtype"):
            fused._bwd(saved, torch.zeros(1, 2, 64, dtype=bad))
    with pytest.raises(TypeError, match="one dtype"):                # and a 16-bit gradient on a float32 forward
        fused._bwd({"t": (torch.zeros(1, 5, 64), torch.zeros(1, 2, 64), idx, torch.zeros(64, 64), torch.zeros(1, 2, 64, dtype=torch.uint8)),
                    "dims": (1, 5, 2, 16, 64)}, torch.zeros(1, 2, 64, dtype=dt))
    assert recorded == []


def test_supported_is_false_for_float64_and_for_host_tensors():
    idx = torch.zeros(1, 2, 16, dtype=torch.int32)
    for dt in (torch.float64, torch.float32, torch.float16, torch.bfloat16):
        assert fused.supported(torch.zeros(1, 5, 64, dtype=dt), idx) is False                 # host tensors: never

    class _Dev:                                                                               # a device tensor, as far as supported() looks
        is_cuda, shape = True, (1, 5, 64)

        def __init__(self, dtype):
            self.dtype = dtype

        def dim(self):
            return 3
    assert fused.supported(_Dev(torch.float64), idx) is False
    assert fused.supported(_Dev(torch.float16), idx) is True and fused.supported(_Dev(torch.bfloat16), idx) is True
