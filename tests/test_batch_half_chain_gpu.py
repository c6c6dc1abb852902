"""GPU, wiring only: a PointnetSAModuleMSG and a PointnetFPModule of pointnet2_batch/pointnet2_modules.py after .to(float16 / bfloat16)
run on 16-bit features end to end - the groupers hand 16-bit tensors to the MLPs, every output and gradient is 16-bit, finite and
non-zero, and what the grouping and the interpolation produce equals, bit for bit, the same chain with each op replaced by
widen -> fp32 op -> round.  The modules themselves needed no change."""
import numpy as np
import pytest
import torch

from batch_half_util import DTYPES, bits, dtype_id, missing_symbols
from pcdet.ops.pointnet2.pointnet2_batch import pointnet2_modules as bmod
from pcdet.ops.pointnet2.pointnet2_batch import pointnet2_utils as bu

pytestmark = pytest.mark.gpu
B, N, NPOINT, C = 3, 40, 12, 8


@pytest.fixture(autouse=True)
def _needs_the_16_bit_entry_points():
    missing = missing_symbols()
    assert not missing, "libfv2p_ops.so lacks %s: nothing is launched" % ", ".join(missing)


def _widened(op):
    """`op` with 16-bit features widened to fp32 before it and its result rounded after it."""
    def run(features, *rest):
        return op(features.float(), *rest).to(features.dtype) if features.dtype in DTYPES else op(features, *rest)
    return run


def _run_chain(sa, fp, xyz, new_xyz, feats, monkeypatch, widen):
    """-> (grouper outputs, interpolation outputs, sa output, fp output); `widen` swaps the ops for their fp32 round trips."""
    seen_group, seen_interp = [], []
    group, interp = (_widened(bu.grouping_operation), _widened(bu.three_interpolate)) if widen else (bu.grouping_operation, bu.three_interpolate)

    def recording_interp(*args):
        seen_interp.append(interp(*args))
        return seen_interp[-1]
    hooks = [g.register_forward_hook(lambda mod, inp, out: seen_group.append(out)) for g in sa.groupers]
    with monkeypatch.context() as mp:
        mp.setattr(bu, "grouping_operation", group)
        mp.setattr(bu, "three_interpolate", recording_interp)
        _, pooled = sa(xyz, feats, new_xyz)                                  # (B, 32, NPOINT)
        spread = fp(xyz, new_xyz, feats, pooled[:, :16].contiguous())        # 16 interpolated + C skip channels = 24
    for h in hooks:
        h.remove()
    return seen_group, seen_interp, pooled, spread


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_sa_and_fp_modules_run_on_16_bit_features(gpu, dtype, monkeypatch):
    torch.manual_seed(3)
    rng = np.random.default_rng(3)
    sa = bmod.PointnetSAModuleMSG(npoint=NPOINT, radii=[0.8, 1.6], nsamples=[4, 8], mlps=[[C, 16], [C, 16]], use_xyz=True).to(gpu).to(dtype)
    fp = bmod.PointnetFPModule(mlp=[24, 16]).to(gpu).to(dtype)
    xyz = torch.from_numpy(rng.random((B, N, 3)).astype(np.float32) * 2).to(gpu)
    new_xyz = xyz[:, :NPOINT].contiguous()
    feats = torch.from_numpy(rng.standard_normal((B, C, N))).to(dtype).to(gpu).requires_grad_(True)
    groups, interps, pooled, spread = _run_chain(sa, fp, xyz, new_xyz, feats, monkeypatch, widen=False)
    assert [tuple(g.shape) for g in groups] == [(B, 3 + C, NPOINT, 4), (B, 3 + C, NPOINT, 8)] and all(g.dtype == dtype for g in groups)
    assert len(interps) == 1 and interps[0].dtype == dtype and interps[0].shape == (B, 16, N)
    assert pooled.shape == (B, 32, NPOINT) and spread.shape == (B, 16, N)
    (pooled.float().square().mean() + spread.float().square().mean()).backward()
    grads = [feats.grad] + [p.grad for m in (sa, fp) for p in m.parameters()]
    for t in [pooled, spread] + grads:
        assert t is not None and t.dtype == dtype and bool(torch.isfinite(t.float()).all()) and bool((t != 0).any())
    # the same chain with every grouping / interpolation done in fp32 on the widened tensor and rounded back
    with torch.no_grad():
        ref_groups, ref_interps, _, _ = _run_chain(sa, fp, xyz, new_xyz, feats, monkeypatch, widen=True)
    for got, ref in zip(groups + interps, ref_groups + ref_interps):
        assert ref.dtype == dtype and np.array_equal(bits(got), bits(ref))
