"""The fused grid set-abstraction on float16 / bfloat16 rows (csrc/sa_fused.hip) on the GPU, against the kernel's stated arithmetic
in float64 (tests/sa_half_cases.py): a derived forward bound, the arg-max byte, the three gradients routed by that byte, exact-integer
cases bit for bit, a centre whose maximum is 0, run-to-run and side-stream bit equality, the untouched float32 route, and the harness's
sa_msg_grid under autocast.  Every bound comes from the number formats; the figures are printed before they are asserted."""
import contextlib

import pytest
import torch

import fv2p_native as _nat
import pcdet.ops as ops
from pcdet.ops.pointnet2.pointnet2_batch import fused
from pcdet.ops.pointnet2.pointnet2_batch import pointnet2_utils as bu

import sa_half_cases as cases

pytestmark = pytest.mark.gpu

CASES = [(sh, dt, w32) for sh in cases.SHAPES for dt in cases.DTYPES for w32 in (False, True)]
case_id = lambda p: "%s-%s-%s" % (cases.shape_id(p[0]), cases.dtype_id(p[1]), "w32" if p[2] else "w16")
_RUNS = {}


def run(c, w32, gpu, go=None, pc=None):
    """Forward and backward of the 16-bit op on a case's operands -> dict of host tensors (out, arg, grad_point, grad_centre, grad_w2)."""
    pp = c["pp"].to(gpu).requires_grad_(True)
    pcd = (c["pc"] if pc is None else pc).to(gpu).requires_grad_(True)
    w2 = (c["w2"] if w32 else c["w2h"]).to(gpu).requires_grad_(True)
    idx = c["idx"].to(gpu)
    assert fused.supported(pp, idx)
    saved = {}
    out = fused._fwd(saved, pp, pcd, idx, w2)
    gp, gc, _, gw = fused._bwd(saved, (c["go"] if go is None else go).to(gpu))
    torch.cuda.synchronize()
    return dict(out=out.cpu(), arg=saved["t"][4].cpu(), grad_point=gp.cpu(), grad_centre=gc.cpu(), grad_w2=gw.cpu())


def shared_run(p, gpu):
    """One GPU run per case, shared by the tests that read it (never modified)."""
    if p not in _RUNS:
        _RUNS[p] = run(cases.case(p[0], p[1]), p[2], gpu)
    return _RUNS[p]


def grouped_route(c, gpu):
    """Today's 16-bit route: grouping_operation, 1x1 product, ReLU, amax on 16-bit tensors -> (r, m, 64) host tensor."""
    pp, pc, w2, idx = c["pp"].to(gpu), c["pc"].to(gpu), c["w2h"].to(gpu), c["idx"].to(gpu)
    grouped = bu.grouping_operation(pp.transpose(1, 2).contiguous(), idx)
    h1 = torch.relu(grouped - pc.transpose(1, 2).unsqueeze(-1))
    h2 = torch.relu(torch.einsum("oc,rcms->roms", w2, h1))
    return h2.amax(dim=-1).transpose(1, 2).cpu()


@pytest.mark.parametrize("p", CASES, ids=case_id)
def test_forward_stays_inside_the_derived_bound(gpu, p):
    c = cases.case(p[0], p[1])
    got = shared_run(p, gpu)
    assert got["out"].dtype == p[1] and got["out"].shape == c["out"].shape
    bound = cases.forward_bound(c)
    ratio = float(((got["out"].double() - c["out"]).abs() / bound).max())
    old = float(((grouped_route(c, gpu).double() - c["out"]).abs() / bound).max())
    print(f"\n{case_id(p)}: forward max |err| / bound = {ratio:.3f}   (the grouped 16-bit route against the same reference: {old:.3f}, not asserted)")
    assert ratio <= 1.0


@pytest.mark.parametrize("p", CASES, ids=case_id)
def test_arg_names_the_earliest_slot_of_the_winning_point(gpu, p):
    c = cases.case(p[0], p[1])
    got = shared_run(p, gpu)
    s = p[0][3]
    arg, out = got["arg"].long(), got["out"].double()
    sets = cases.arg_sets(c)
    strict, want, e = sets["strict"], sets["want"], c["e"]
    share = float((~strict).double().mean())
    print(f"\n{case_id(p)}: near-tie share {share:.2e} ({int((~strict).sum())} of {strict.numel()} pairs)")
    assert share <= 1e-3
    assert bool(((arg == 255) == (out == 0)).all()) and bool(((arg == 255) | (arg < s)).all())
    assert bool((arg[strict] == want[strict]).all()), int((arg[strict] != want[strict]).sum())
    # near-ties: a sample whose reference value is within 2 e of the maximum (255: a maximum within 2 e of zero)
    near = ~strict
    picked = torch.gather(c["a"], 2, arg.clamp(max=s - 1).unsqueeze(2)).squeeze(2)
    ok = torch.where(arg == 255, sets["v1"] <= 2 * e, picked >= sets["v1"] - 2 * e)
    assert bool(ok[near].all())


@pytest.mark.parametrize("p", CASES, ids=case_id)
def test_gradients_stay_inside_the_derived_bounds(gpu, p):
    c = cases.case(p[0], p[1])
    got = shared_run(p, gpu)
    refs = cases.backward_ref(c, got["arg"].long(), p[2])          # routed by the kernel's own arg (validated above)
    want_dtype = {"grad_point": p[1], "grad_centre": p[1], "grad_w2": torch.float32 if p[2] else p[1]}
    worst = {}
    for name, (ref, bound) in refs.items():
        assert got[name].dtype == want_dtype[name] and got[name].shape == ref.shape, name
        worst[name] = float(((got[name].double() - ref).abs() / bound).max())
    print(f"\n{case_id(p)}: max |err| / bound  " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("w32", [False, True], ids=["w16", "w32"])
@pytest.mark.parametrize("dt", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("s", [16, 32])
def test_exact_integer_case_is_bit_equal(gpu, s, dt, w32):
    c = cases.exact_case(s)
    half = dict(c, pp=c["pp"].to(dt), pc=c["pc"].to(dt), w2h=c["w2"].to(dt), go=c["go"].to(dt))
    got = run(half, w32, gpu)
    assert torch.equal(got["arg"].long(), c["arg"])
    for name in ("out", "grad_point", "grad_centre"):
        assert got[name].dtype == dt and torch.equal(got[name], c[name].to(dt)), name
    assert torch.equal(got["grad_w2"], c["grad_w2"].to(torch.float32 if w32 else dt))


@pytest.mark.parametrize("on", [False, True], ids=["switch-off", "switch-on"])
@pytest.mark.parametrize("s", [16, 32])
def test_exact_integer_case_is_bit_equal_in_float32(gpu, s, on):
    """The float32 leg of the case above: the float32 kernels on the same operands, with the LDS-atomic backward (fv2p_sa_grid_bwd, switch
    off) and the fixed-order one (fv2p_sa_grid_bwd_gather, switch on) - integer sums are exact in any order -, held to the values the two
    16-bit formats are held to."""
    c = cases.exact_case(s)
    with mode(on):
        got = run(c, True, gpu)
    assert torch.equal(got["arg"].long(), c["arg"])
    for name in ("out", "grad_point", "grad_centre", "grad_w2"):
        assert got[name].dtype == torch.float32 and torch.equal(got[name], c[name].float()), name


@pytest.mark.parametrize("dt", cases.DTYPES, ids=cases.dtype_id)
def test_a_centre_whose_maximum_is_zero(gpu, dt):
    c = cases.case((5, 100, 30, 16), dt)
    k = 7
    pc = c["pc"].clone()
    pc[:, k] = 100.0                                                # h1 = relu(P - 100) = 0 for every sample of centre k
    got = run(c, False, gpu, pc=pc)
    assert bool((got["out"][:, k] == 0).all()) and bool((got["arg"][:, k] == 255).all()) and bool((got["grad_centre"][:, k] == 0).all())
    assert bool((got["out"][:, k - 1] > 0).any())
    only = torch.zeros_like(c["go"])
    only[:, k] = c["go"][:, k]                                      # a gradient that reaches centre k alone: nothing may come back
    got = run(c, False, gpu, go=only, pc=pc)
    for name in ("grad_point", "grad_centre", "grad_w2"):
        assert bool((got[name] == 0).all()), name


@contextlib.contextmanager
def mode(on):
    was = ops.is_deterministic()
    ops.set_deterministic(on)
    try:
        yield
    finally:
        ops.set_deterministic(was)


@pytest.mark.parametrize("on", [False, True], ids=["switch-off", "switch-on"])
@pytest.mark.parametrize("dt", cases.DTYPES, ids=cases.dtype_id)
def test_two_calls_and_a_side_stream_give_identical_bits(gpu, dt, on):
    c = cases.case((3, 512, 216, 32), dt)
    names = ("out", "arg", "grad_point", "grad_centre", "grad_w2")
    with mode(on):
        first = run(c, True, gpu)
        again = run(c, True, gpu)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            other = run(c, True, gpu)
        side.synchronize()
    for name in names:
        assert torch.equal(first[name], again[name]), name
        assert torch.equal(first[name], other[name]), name + " on a side stream"
    ref = shared_run(((3, 512, 216, 32), dt, True), gpu)
    for name in names:
        assert torch.equal(first[name], ref[name]), name + " against the run of the other tests"


class _Recorder:
    """fv2p_native.call with the names of the entry points recorded."""

    def __init__(self, monkeypatch):
        self.names, real = [], _nat.call
        monkeypatch.setattr(_nat, "call", lambda name, *a: (self.names.append(name), real(name, *a))[1])


def test_float32_inputs_still_run_the_float32_kernels(gpu, monkeypatch):
    pp, pc, w2, idx, go = (t.to(gpu) for t in cases.inputs((5, 100, 30, 16)))
    rec = _Recorder(monkeypatch)
    outs = []
    for _ in range(2):
        a, b, w = pp.clone().requires_grad_(True), pc.clone().requires_grad_(True), w2.clone().requires_grad_(True)
        out = fused.sa_grid_max(a, b, idx, w)
        out.backward(go)
        outs.append(out.detach())
        assert out.dtype == torch.float32 and a.grad.dtype == torch.float32 and w.grad.dtype == torch.float32
    assert rec.names == ["fv2p_sa_grid_fwd", "fv2p_sa_grid_bwd"] * 2, rec.names
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("dt", cases.DTYPES, ids=cases.dtype_id)
def test_sa_msg_grid_under_autocast_reaches_the_16_bit_op_with_the_fp32_weight(gpu, dt, monkeypatch):
    from fv2p_harness import fv2p_model as fm
    from pcdet.ops.pointnet2.pointnet2_batch.pointnet2_modules import PointnetSAModuleMSG
    torch.manual_seed(5)
    sa = PointnetSAModuleMSG(npoint=216, radii=[0.8, 1.6], nsamples=[16, 32], mlps=[[32, 64, 64], [32, 64, 64]], use_xyz=True, bn=False).to(gpu)
    g = torch.Generator().manual_seed(11)
    R, N = 4, 128
    xyz = ((torch.rand(R, N, 3, generator=g) * 2 - 1) * 3.0).to(gpu)                 # RoI-local coordinates within +-3 m
    feats = torch.randn(R, 32, N, generator=g).to(gpu)
    axis = torch.linspace(-2.5, 2.5, 6)
    centres = torch.stack(torch.meshgrid(axis, axis, axis, indexing="ij"), -1).reshape(1, 216, 3).repeat(R, 1, 1).to(gpu)
    want = fm.sa_msg_grid(sa, xyz, feats, centres).detach()                          # the fp32 run
    rec = _Recorder(monkeypatch)
    with torch.autocast("cuda", dt):
        out = fm.sa_msg_grid(sa, xyz, feats, centres)
    assert rec.names.count("fv2p_sa_grid_fwd_h") == 2 and "fv2p_sa_grid_fwd" not in rec.names, rec.names      # once per radius
    assert not [n for n in rec.names if n.startswith("fv2p_group_points")], rec.names
    assert out.dtype == dt and out.shape == want.shape
    out.float().square().sum().backward()
    assert rec.names.count("fv2p_sa_grid_bwd_h") == 2
    for prm in sa.parameters():
        assert prm.grad is not None and prm.grad.dtype == torch.float32 and bool(torch.isfinite(prm.grad).all()) and float(prm.grad.abs().max()) > 0
    monkeypatch.setattr(fused, "supported", lambda *a, **k: False)                   # today's route under the same autocast
    with torch.autocast("cuda", dt), torch.no_grad():
        old = fm.sa_msg_grid(sa, xyz, feats, centres)
    E = float((old.float() - want).abs().max())
    err = float((out.detach().float() - want).abs().max())
    print(f"\n{cases.dtype_id(dt)}: |autocast fused - fp32| = {err:.3e}, today's route E = {E:.3e}")
    assert err <= 2 * E + 1e-6
