"""The stacked pointnet2 HIP ops (csrc/pointnet2.hip: ball_query_stack_k, voxel_query_stack_k, three_nn_stack_k and its grid form,
group_points_stack_k / _grad_k, three_interp_stack_k / _grad_k and the gather forms of both gradients) through
pcdet.ops.pointnet2.pointnet2_stack, against BOTH the plain numpy references of tests/stack_cases.py and the oracle, on every case of
the builder: zero-query and zero-point samples, workgroups that span 37 samples, query totals around 64 and 256, samples that end on and
one past a 1024-point tile, nsample 1 ... 100, channels 1 ... 128, exact ties and exact d2 == r2 on the dyadic lattice
(tests/test_pointnet2_stack_cpu.py proves cases and references on the host).

Bounds, none of them measured:
* indices, empty masks, grouped features, 3-NN squared distances: 0;
* generic family against the float64 brute force: only queries with a candidate within 4 * 2^-24 * max(d2, r2) of the deciding threshold
  are left out (at most 1 % per case, enforced by the CPU file); the float32 reference covers every query bit for bit;
* interpolation: |got - ref64| <= 4 * 2^-24 * sum_j |w_j f_j| per element (three products, two additions);
* gradients: |got - ref64| <= (k + 2) * 2^-24 * S per destination element, k contributions of absolute sum S - the bound of a float32 sum
  in any order, so the atomic and the gather form share it; the gather forms are also bit-identical between two calls.

tests/test_pointnet2_gpu.py::test_stack_ops compares the interpolation with a float32 torch expression at an absolute 1e-5.  It stays as
it is; the float64 bound here supersedes it - do not "fix" that test by widening it."""
import contextlib

import numpy as np
import pytest
import torch

import oracle
import pcdet.ops as ops
import stack_cases as sc
from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils as su
from pcdet.ops.pointnet2.pointnet2_stack import voxel_query_utils as vq

pytestmark = pytest.mark.gpu
U = sc.U32


def T(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


@contextlib.contextmanager
def deterministic_mode():
    """The route of tests/test_deterministic_gpu.py: with the mode on, the autograd ops take the gather forms of their gradients."""
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        yield
    finally:
        ops.set_deterministic(was)


def zeroed(raw):
    """Raw op output -> (idx with empty balls as row 0, empty mask): what the Python wrappers return."""
    empty = raw[:, 0] == -1
    idx = raw.copy()
    idx[empty] = 0
    return idx, empty


def within(got, want, bound, what):
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"{what}: largest error / bound = {worst:.3f}")
    assert (err <= bound).all(), f"{what}: {int((err > bound).sum())} elements outside the bound, worst ratio {worst:.3f}"


@pytest.mark.parametrize("case", sc.BALL_CASES, ids=sc.case_id)
def test_ball_query_stack(gpu, case):
    layout, family, radius, nsample = case
    c = sc.cloud_case(layout, family, radius)
    ref32, _ = sc.ref_ball_query(c, nsample, sc.d2_f32)
    ref64, _ = sc.ref_ball_query(c, nsample, sc.d2_f64)
    idx, empty = su.ball_query(radius, nsample, T(c["xyz"], gpu), T(c["xyz_cnt"], gpu), T(c["new_xyz"], gpu), T(c["new_cnt"], gpu))
    assert idx.dtype == torch.int32 and tuple(idx.shape) == ref32.shape
    got, got_empty = idx.cpu().numpy(), empty.cpu().numpy()
    for ref in (ref32, oracle.ball_query_stack(radius, nsample, c["xyz"], c["xyz_cnt"], c["new_xyz"], c["new_cnt"])):
        want, want_empty = zeroed(ref)
        assert np.array_equal(got_empty, want_empty) and np.array_equal(got, want)
    keep = np.ones(got.shape[0], bool) if family == "lattice" else ~sc.ambiguous_ball(c)
    want, want_empty = zeroed(ref64)
    assert np.array_equal(got[keep], want[keep]) and np.array_equal(got_empty[keep], want_empty[keep])


@pytest.mark.parametrize("case", sc.VOXEL_CASES, ids=sc.case_id)
def test_voxel_query_stack(gpu, case):
    family, max_range, radius, nsample = case
    s = sc.voxel_scene(family, radius)
    ref32, _ = sc.ref_voxel_query(s, max_range, nsample, sc.d2_f32)
    ref64, _ = sc.ref_voxel_query(s, max_range, nsample, sc.d2_f64)
    Z, Y, X = sc.GRID
    zyx = s["new_coords"][:, 1:]
    assert (zyx >= 0).all() and (zyx < [Z, Y, X]).all() and (s["new_coords"][:, 0] < 3).all() and s["vol"].max() < s["xyz"].shape[0]
    idx, empty = vq.voxel_query(list(max_range), radius, nsample, T(s["xyz"], gpu), T(s["new_xyz"], gpu), T(s["new_coords"], gpu), T(s["vol"], gpu))
    got, got_empty = idx.cpu().numpy(), empty.cpu().numpy()
    for ref in (ref32, oracle.voxel_query_stack(list(max_range), radius, nsample, s["xyz"], s["new_xyz"], s["new_coords"], s["vol"])):
        want, want_empty = zeroed(ref)
        assert np.array_equal(got_empty, want_empty) and np.array_equal(got, want)
    keep = np.ones(got.shape[0], bool) if family == "lattice" else ~sc.ambiguous_voxel(s, max_range)
    want, want_empty = zeroed(ref64)
    assert np.array_equal(got[keep], want[keep]) and np.array_equal(got_empty[keep], want_empty[keep])


@pytest.mark.parametrize("case", sc.NN_CASES, ids=sc.case_id)
def test_three_nn_stack(gpu, case):
    """Fewer than three known points in a sample: the untouched slots hold (+inf, the sample's first global row) - the rule of the
    reference's three_nn_kernel_stack, stated in stack_cases.ref_three_nn."""
    layout, family = case
    c = sc.cloud_case(layout, family)
    rd32, ri32 = sc.ref_three_nn(c, sc.d2_f32)
    _, ri64 = sc.ref_three_nn(c, sc.d2_f64)
    dist, idx = su.three_nn(T(c["new_xyz"], gpu), T(c["new_cnt"], gpu), T(c["xyz"], gpu), T(c["xyz_cnt"], gpu))
    got_d, got_i = dist.cpu().numpy(), idx.cpu().numpy()
    assert got_i.dtype == np.int32 and got_d.dtype == np.float32
    od, oi = oracle.three_nn_stack(c["new_xyz"], c["new_cnt"], c["xyz"], c["xyz_cnt"])
    for d2, ref in ((rd32, ri32), (od, oi)):
        assert np.array_equal(got_i, ref)
        assert np.array_equal(got_d, np.sqrt(d2))          # the wrapper returns distances: the correctly rounded root of the same d2
    keep = np.ones(got_i.shape[0], bool) if family == "lattice" else ~sc.ambiguous_three_nn(c)
    assert np.array_equal(got_i[keep], ri64[keep])


@pytest.mark.parametrize("case", sc.GROUP_CASES, ids=sc.case_id)
def test_group_points_stack_and_its_gradients(gpu, case):
    layout, family, radius, nsample, channels = case
    c = sc.cloud_case(layout, family, radius)
    local, _ = zeroed(sc.ref_ball_query(c, nsample, sc.d2_f32)[0])
    rows = sc.global_rows(c, local)
    n, m = c["xyz"].shape[0], rows.shape[0]
    assert rows.min() >= 0 and rows.max() < n                      # every row the kernels will read or add to exists
    rng = np.random.default_rng(n + m + channels)
    feats = rng.standard_normal((n, channels)).astype(np.float32)
    go = rng.standard_normal((m, channels, nsample)).astype(np.float32)
    cnt, qcnt, idx_t, go_t = T(c["xyz_cnt"], gpu), T(c["new_cnt"], gpu), T(local, gpu), T(go, gpu)

    def grad():
        ft = T(feats, gpu).requires_grad_(True)
        out = su.grouping_operation(ft, cnt, idx_t, qcnt)
        out.backward(go_t)
        return out.detach().cpu().numpy(), ft.grad.cpu().numpy()

    out, g_atomic = grad()
    assert np.array_equal(out, sc.ref_group(feats, rows))          # pure indexing: bit for bit
    want, mag, k = sc.ref_group_grad(go, rows, n)
    bound = (k[:, None] + 2) * U * mag
    within(g_atomic, want, bound, f"grouping gradient, atomic form, up to {int(k.max())} contributions")
    with deterministic_mode():
        _, g1 = grad()
        _, g2 = grad()
    assert np.array_equal(g1.view(np.uint32), g2.view(np.uint32))  # fixed order: equal bits
    within(g1, want, bound, "grouping gradient, gather form")


@pytest.mark.parametrize("case", sc.INTERP_CASES, ids=sc.case_id)
def test_three_interpolate_stack_and_its_gradients(gpu, case):
    layout, family, channels = case
    c = sc.cloud_case(layout, family)
    _, idx = sc.ref_three_nn(c, sc.d2_f32)
    m, n = c["xyz"].shape[0], idx.shape[0]
    assert idx.min() >= 0 and idx.max() < m                        # an untouched slot of a point-less LAST sample would point behind the rows
    rng = np.random.default_rng(m + n + channels)
    w = rng.random((n, 3)).astype(np.float32)
    w = (w / w.sum(1, keepdims=True)).astype(np.float32)
    feats = rng.standard_normal((m, channels)).astype(np.float32)
    go = rng.standard_normal((n, channels)).astype(np.float32)
    idx_t, w_t, go_t = T(idx, gpu), T(w, gpu), T(go, gpu)

    def grad():
        ft = T(feats, gpu).requires_grad_(True)
        out = su.three_interpolate(ft, idx_t, w_t)
        out.backward(go_t)
        return out.detach().cpu().numpy(), ft.grad.cpu().numpy()

    out, g_atomic = grad()
    want, mag = sc.ref_interp(feats, idx, w)
    within(out, want, 4 * U * mag, "interpolation")
    want, mag, k = sc.ref_interp_grad(go, idx, w, m)
    bound = (k[:, None] + 2) * U * mag
    within(g_atomic, want, bound, f"interpolation gradient, atomic form, up to {int(k.max())} contributions")
    with deterministic_mode():
        _, g1 = grad()
        _, g2 = grad()
    assert np.array_equal(g1.view(np.uint32), g2.view(np.uint32))
    within(g1, want, bound, "interpolation gradient, gather form")
