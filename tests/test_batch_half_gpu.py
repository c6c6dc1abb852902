"""GPU: the batch gather / grouping / interpolation on float16 / bfloat16 features (csrc/pointnet2.hip, the 16-bit form of
csrc/scatter_add.hip), through the Python ops, the ext-module wrappers and the raw entry points.

  copies (gather, grouping forward): bit-equal to the fp32 op on the widened input, rounded back; an index outside [0, n) gives zeros;
  interpolation forward: bit-equal to the fp32 op on the widened features, rounded; integer features in [-8, 8] with weights from
      {0, 1/4, 1/2, 1} are exact; random inputs satisfy
      |out - ref64| <= 2^-(p+1) |ref64| + 4 * 2^-24 * sum |w_i| |f_i| + 2^-25      (p = 10 fp16, 7 bf16; ref64 from the widened inputs):
      one final rounding, plus three products and two sums in fp32 (each within 2^-24 of a magnitude below the sum of the terms);
  gradients (fixed order, fp32 sums, one rounding): an element of k entries is within 2^-(p+1) |ref64| + (k + 2) 2^-24 sum |terms|
      (k products and fewer than k sums, whatever the association), exact on integer inputs, 0 where no entry reaches in a NaN-filled
      output, entries outside the range dropped, two streams bit-identical, and the bits of the fp32 *_grad_gather entry point on the
      widened gradient, rounded;
  float64 and 16-bit coordinates raise TypeError; float32 keeps going to the fp32 entry points, bit for bit."""
import numpy as np
import pytest
import torch

import fv2p_native as nat
from batch_half_util import DT_CODE, DTYPES, PREC, bits, dtype_id, f64, missing_symbols, round_to
from pcdet.ops.pointnet2.pointnet2_batch import pointnet2_batch_cuda as ext
from pcdet.ops.pointnet2.pointnet2_batch import pointnet2_utils as bu

pytestmark = pytest.mark.gpu
CHANNELS = [8, 5, 64]
B, N = 2, 40                       # samples, feature points (known rows of the interpolation)
GROUP_SHAPES = [(15, 16), (7, 5)]  # (M, S): row length 240 (the 16-byte path) and 35 (the element path)
GATHER_M = [64, 77]
QUERIES = [80, 77]
EPS24 = 2.0 ** -24
WEIGHTS = np.array([0.0, 0.25, 0.5, 1.0])


@pytest.fixture(autouse=True)
def _needs_the_16_bit_entry_points():
    missing = missing_symbols()
    assert not missing, "libfv2p_ops.so lacks %s: nothing is launched" % ", ".join(missing)


def _t(a, dtype, gpu):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dtype).to(gpu)


def _i(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(gpu)


def _w(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(gpu)


# ---- index lists shared by the tests (built once, never changed) ------------------------------------------------------------------
def _grad_entries(seed, total, hub, full, empty):
    """`total` entries of one sample into N rows: row `hub` 100 times, row `full` exactly 32 times, the rows of `empty` never, one
    entry past the end, the rest spread over the other rows; shuffled."""
    rng = np.random.default_rng(seed)
    others = [r for r in range(N) if r not in (hub, full) and r not in empty]
    flat = np.concatenate([np.full(100, hub), np.full(32, full), [N + 3], rng.choice(others, size=total - 133)]).astype(np.int64)
    rng.shuffle(flat)
    return flat


def _grad_case(total, seed):
    """Two samples with different hubs, full rows and empty rows."""
    return np.stack([_grad_entries(seed, total, 0, 28, (5, 6, 39)), _grad_entries(seed + 1, total, 7, 3, (0, 11, 12, 30))])


GROUP_IDX = _grad_case(240, 21)                 # (2, 240) = idx (2, 15, 16), and the gather's (2, 240)
INTERP_IDX = _grad_case(231, 31)                # (2, 231) = idx (2, 77, 3)


def _fwd_idx(seed, per, far):
    """(B, per) random rows of [0, N), another pattern per sample; `far` puts one index >= N into every sample."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, N, size=(B, per))
    if far:
        for b in range(B):
            idx[b, (7 + 11 * b) % per] = N + b
    return idx


def test_the_fixtures_hold_what_the_checks_need():
    for case in (GROUP_IDX, INTERP_IDX):
        assert not np.array_equal(case[0], case[1])
        for flat in case:
            cnt = np.bincount(flat[flat < N], minlength=N)
            assert cnt.max() == 100 and 32 in cnt.tolist() and (cnt == 0).sum() >= 3 and (flat >= N).sum() == 1 and flat.size % 32 != 0
    assert GROUP_SHAPES[0][0] * GROUP_SHAPES[0][1] == GROUP_IDX.shape[1] and GROUP_IDX.shape[1] % 8 == 0
    assert (GROUP_SHAPES[1][0] * GROUP_SHAPES[1][1]) % 8 and QUERIES[0] % 8 == 0 and QUERIES[1] % 8 and GATHER_M[0] % 8 == 0 and GATHER_M[1] % 8
    assert 3 * QUERIES[1] == INTERP_IDX.shape[1]
    for per in (35, 64, 240):
        far = _fwd_idx(1, per, True)
        assert ((far >= N).sum(1) == 1).all() and (_fwd_idx(1, per, False) < N).all()


# ---- copies ---------------------------------------------------------------------------------------------------------------------
def _check_copy(out, ref, raw, far_np, c, dtype):
    assert out.dtype == dtype and out.shape == ref.shape and np.array_equal(bits(out), bits(ref.to(dtype)))
    far = torch.from_numpy(far_np).to(out.device)[:, None, :].expand(-1, c, -1).reshape(out.shape)
    assert int(far.sum()) == B * c
    assert torch.equal(raw[~far].view(torch.int16), out[~far].view(torch.int16)) and bool((raw[far] == 0).all())


@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_grouping_forward_is_a_copy(gpu, dtype, c):
    f = _t(np.random.default_rng(c).standard_normal((B, c, N)), dtype, gpu)
    for m, s in GROUP_SHAPES:
        far_np = _fwd_idx(100 + m, m * s, True)
        idx, far = _i(np.minimum(far_np, N - 1).reshape(B, m, s), gpu), _i(far_np.reshape(B, m, s), gpu)   # the fp32 kernel never sees the far index
        out = bu.grouping_operation(f, idx)
        assert out.shape == (B, c, m, s)
        raw = torch.full((B, c, m, s), float("nan"), dtype=dtype, device=gpu)
        nat.call("fv2p_group_points_batch_h", B, c, N, m, s, f, far, raw, DT_CODE[dtype], nat.stream())
        _check_copy(out, bu.grouping_operation(f.float(), idx), raw, far_np >= N, c, dtype)


@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_gather_forward_is_a_copy(gpu, dtype, c):
    f = _t(np.random.default_rng(10 + c).standard_normal((B, c, N)), dtype, gpu)
    for m in GATHER_M:
        far_np = _fwd_idx(200 + m, m, True)
        idx, far = _i(np.minimum(far_np, N - 1), gpu), _i(far_np, gpu)
        out = bu.gather_operation(f, idx)
        assert out.shape == (B, c, m)
        raw = torch.full((B, c, m), float("nan"), dtype=dtype, device=gpu)
        nat.call("fv2p_gather_points_h", B, c, N, m, f, far, raw, DT_CODE[dtype], nat.stream())
        _check_copy(out, bu.gather_operation(f.float(), idx), raw, far_np >= N, c, dtype)


# ---- interpolation forward -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_interpolation_forward(gpu, dtype, c):
    rng = np.random.default_rng(300 + c)
    for n in QUERIES:
        far_np = _fwd_idx(300 + n, 3 * n, True).reshape(B, n, 3)
        safe_np = np.minimum(far_np, N - 1)
        for exact in (True, False):
            f64_ = rng.integers(-8, 9, size=(B, c, N)).astype(np.float64) if exact else round_to(rng.standard_normal((B, c, N)), dtype)
            w64 = rng.choice(WEIGHTS, size=(B, n, 3)) if exact else rng.random((B, n, 3)).astype(np.float32).astype(np.float64)
            f, w = _t(f64_, dtype, gpu), _w(w64, gpu)
            out = bu.three_interpolate(f, _i(safe_np, gpu), w)
            assert out.dtype == dtype and out.shape == (B, c, n)
            assert np.array_equal(bits(out), bits(bu.three_interpolate(f.float(), _i(safe_np, gpu), w).to(dtype)))
            if exact:                                                                          # a 16-bit weight is widened, not misread
                assert np.array_equal(bits(out), bits(bu.three_interpolate(f, _i(safe_np, gpu), w.to(dtype))))
            # the raw entry point on a NaN-filled output; the known index past the end counts as a row of zeros
            raw = torch.full((B, c, n), float("nan"), dtype=dtype, device=gpu)
            nat.call("fv2p_three_interpolate_batch_h", B, c, N, n, f, _i(far_np, gpu), w, raw, DT_CODE[dtype], nat.stream())
            picked = np.stack([f64_[b][:, safe_np[b]] for b in range(B)])                       # [B, c, n, 3]
            terms = np.where((far_np < N)[:, None], w64[:, None] * picked, 0.0)
            ref64, mag = terms.sum(-1), np.abs(terms).sum(-1)
            near = np.broadcast_to((far_np < N).all(-1)[:, None, :], (B, c, n))                # queries without the far index
            assert (~near).sum() == B * c and np.array_equal(bits(raw)[near], bits(out)[near])
            if exact:
                assert np.array_equal(f64(raw), round_to(ref64, dtype))
            else:
                bound = 2.0 ** -(PREC[dtype] + 1) * np.abs(ref64) + 4 * EPS24 * mag + 2.0 ** -25
                err = np.abs(f64(raw) - ref64)
                print("three_interpolate (batch) n=%d: max err / bound = %.3f" % (n, (err / bound).max()))
                assert (err <= bound).all()


# ---- gradients ----------------------------------------------------------------------------------------------------------------------
def _scatter_ref(dst, n_rows, coef, src64):
    """float64 reference of a scatter-add, the sum of |terms| and the entry count per row; entries outside [0, n_rows) are dropped."""
    keep = (dst >= 0) & (dst < n_rows)
    terms = coef[keep, None] * src64[keep]
    ref, mag = np.zeros((n_rows, src64.shape[1])), np.zeros((n_rows, src64.shape[1]))
    np.add.at(ref, dst[keep], terms)
    np.add.at(mag, dst[keep], np.abs(terms))
    return ref, mag, np.bincount(dst[keep], minlength=n_rows).astype(np.float64)[:, None]


def _batch_ref(flat, coef, g64, div):
    """grad_out g64 [B, c, P], entries flat [B, div * P] (entry j reads column j // div) -> (ref, mag, k) as [B, c, N] arrays."""
    outs = []
    for b in range(B):
        src = g64[b].T[np.arange(flat.shape[1]) // div]                                       # entry -> its c gradients
        outs.append([a.T for a in _scatter_ref(flat[b], N, coef[b], src)])
    return [np.stack([o[k] for o in outs]) for k in range(3)]


def _on_two_streams(fn):
    outs = []
    for _ in range(2):
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            outs.append(fn())
        st.synchronize()
    return outs


def _raw_grad(op, sizes, g, lists, dtype, gpu):
    """The 16-bit entry point `op`_h on a NaN-filled grad_points [B, c, N]."""
    out = torch.full((B, g.shape[1], N), float("nan"), dtype=dtype, device=gpu)
    ws = nat.workspace(getattr(nat.lib(), op + "_h_ws_bytes")(*sizes), gpu)
    nat.call(op + "_h", *sizes, g, *lists, out, DT_CODE[dtype], ws, ws.numel(), nat.stream())
    return out


def _fp32_grad(op, sizes, g, lists, gpu):
    """The fp32 fixed-order entry point `op`_gather on the widened gradient."""
    out = torch.full((B, g.shape[1], N), float("nan"), dtype=torch.float32, device=gpu)
    ws = nat.workspace(getattr(nat.lib(), op + "_ws_bytes")(*sizes), gpu)
    nat.call(op + "_gather", *sizes, g.float(), *lists, out, ws, ws.numel(), nat.stream())
    return out


def _check_grad(op, sizes, shape, flat, div, apply, dtype, c, gpu, seed):
    """Every check of one gradient: `flat` [B, entries] the index lists with their far entry, `apply(feats, idx, w)` the Python op."""
    rng = np.random.default_rng(seed)
    idx_shape = (B,) + shape[2:] + ((3,) if div == 3 else ())
    idx, safe = _i(flat.reshape(idx_shape), gpu), _i(np.minimum(flat, N - 1).reshape(idx_shape), gpu)
    for exact in (True, False):
        g64 = rng.integers(-8, 9, size=shape).astype(np.float64) if exact else round_to(rng.standard_normal(shape), dtype)
        if div == 3:
            w64 = rng.choice(WEIGHTS, size=flat.shape) if exact else rng.random(flat.shape).astype(np.float32).astype(np.float64)
            w = [_w(w64.reshape(idx_shape), gpu)]
        else:
            w64, w = np.ones(flat.shape), []
        g = _t(g64, dtype, gpu)
        a, b = _on_two_streams(lambda: _raw_grad(op, sizes, g, [idx] + w, dtype, gpu))
        assert np.array_equal(bits(a), bits(b))
        ref64, mag, k = _batch_ref(flat, w64, g64.reshape(B, c, -1), div)
        got = f64(a)
        untouched = np.broadcast_to(k == 0, got.shape)
        assert (k[0] == 0).sum() >= 3 and (k[1] == 0).sum() >= 3 and (got[untouched] == 0).all()
        if exact:
            assert np.abs(ref64).max() < 2048 and np.array_equal(got, round_to(ref64, dtype))
        else:
            bound = 2.0 ** -(PREC[dtype] + 1) * np.abs(ref64) + (k + 2) * EPS24 * mag
            err = np.abs(got - ref64)
            print("%s_h: max err / bound = %.3f" % (op, (err / np.maximum(bound, 1e-300)).max()))
            assert np.isfinite(got).all() and (err <= bound).all()
        # the bits of the fp32 fixed-order form on the widened gradient, rounded (in-range indices only: the far entry clamped)
        mine = _raw_grad(op, sizes, g, [safe] + w, dtype, gpu)
        assert np.array_equal(bits(mine), bits(_fp32_grad(op, sizes, g, [safe] + w, gpu).to(dtype)))
        # the autograd route reaches the same entry point, whatever the deterministic switch says
        feats = torch.zeros((B, c, N), dtype=dtype, device=gpu, requires_grad=True)
        for det in (False, True):
            nat.set_deterministic(det)
            try:
                feats.grad = None
                apply(feats, safe, *w).backward(g)
            finally:
                nat.set_deterministic(False)
            assert feats.grad.dtype == dtype and np.array_equal(bits(feats.grad), bits(mine))


@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_grouping_gradient(gpu, dtype, c):
    m, s = GROUP_SHAPES[0]
    _check_grad("fv2p_group_points_batch_grad", (B, c, N, m, s), (B, c, m, s), GROUP_IDX, 1, bu.grouping_operation, dtype, c, gpu, 400 + c)


@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_gather_gradient(gpu, dtype, c):
    m = GROUP_IDX.shape[1]
    _check_grad("fv2p_gather_points_grad", (B, c, N, m), (B, c, m), GROUP_IDX, 1, bu.gather_operation, dtype, c, gpu, 500 + c)


@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_interpolation_gradient(gpu, dtype, c):
    n = QUERIES[1]
    _check_grad("fv2p_three_interpolate_batch_grad", (B, c, n, N), (B, c, n), INTERP_IDX, 3, bu.three_interpolate, dtype, c, gpu, 600 + c)


# ---- top3_interpolate on (N, C) rows ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_top3_interpolate_on_16_bit_rows(gpu, dtype):
    rng = np.random.default_rng(7)
    xyz = _w(rng.random((N, 3)) * 4, gpu)
    for c, n in ((8, QUERIES[0]), (5, QUERIES[1])):
        new_xyz = _w(rng.random((n, 3)) * 4, gpu)
        feats = _t(rng.standard_normal((N, c)), dtype, gpu).requires_grad_(True)
        g = _t(rng.standard_normal((n, c)), dtype, gpu)
        out = bu.top3_interpolate(xyz, new_xyz, feats)
        assert out.dtype == dtype and out.shape == (n, c)
        out.backward(g)
        grad, feats.grad = feats.grad, None
        assert grad.dtype == dtype and grad.shape == (N, c) and bool(torch.isfinite(grad.float()).all()) and bool((grad != 0).any())
        # the batch op on the transposed tensor: the same products, sums and rounding
        dist, idx = bu.three_nn(new_xyz.unsqueeze(0).contiguous(), xyz.unsqueeze(0).contiguous())
        via = bu.three_interpolate(feats.t().unsqueeze(0).contiguous(), idx, bu._inverse_distance_weights(dist))[0].t()
        assert np.array_equal(bits(out), bits(via))
        via.backward(g)
        assert np.array_equal(bits(grad), bits(feats.grad))                  # one association (fv2p_scatter_add's) on both routes
        feats.grad = None
        # with gradients to the coordinates: grouped in 16 bits, summed in fp32, one rounding = the fp32 route on the widened rows, rounded
        wg = bu.top3_interpolate_with_grad(xyz, new_xyz, feats)
        assert wg.dtype == dtype and wg.shape == (n, c)
        assert np.array_equal(bits(wg), bits(bu.top3_interpolate_with_grad(xyz, new_xyz, feats.detach().float()).to(dtype)))
        wg.backward(g)
        assert feats.grad.dtype == dtype and bool(torch.isfinite(feats.grad.float()).all()) and bool((feats.grad != 0).any())


# ---- dtypes that are not served, and float32 left alone ---------------------------------------------------------------------------------
def test_unserved_dtypes_raise(gpu):
    from pcdet.ops.roiaware_pool3d.roiaware_pool3d_utils import RoIAwarePool3d
    from pcdet.ops.roipoint_pool3d.roipoint_pool3d_utils import RoIPointPool3d
    c, m, s = 8, 7, 5
    f = torch.zeros((B, c, N), dtype=torch.float64, device=gpu)
    gi, ii = _i(_fwd_idx(1, m * s, False).reshape(B, m, s), gpu), _i(_fwd_idx(2, 3 * m, False).reshape(B, m, 3), gpu)
    w = torch.full((B, m, 3), 0.25, device=gpu)
    msg = "float32, float16 and bfloat16"
    with pytest.raises(TypeError, match=msg):
        bu.grouping_operation(f, gi)
    with pytest.raises(TypeError, match=msg):
        bu.gather_operation(f, gi[:, :, 0].contiguous())
    with pytest.raises(TypeError, match=msg):
        bu.three_interpolate(f, ii, w)
    with pytest.raises(TypeError, match=msg):
        bu._group_grad(dict(shape=(B, c, N, m, s), idx=gi), torch.zeros((B, c, m, s), dtype=torch.float64, device=gpu))
    with pytest.raises(TypeError, match=msg):
        bu._gather_grad(dict(shape=(B, c, N, m), idx=gi), torch.zeros((B, c, m), dtype=torch.float64, device=gpu))
    with pytest.raises(TypeError, match=msg):
        bu._interp_grad(dict(shape=(B, c, N, m), idx=ii, weight=w), torch.zeros((B, c, m), dtype=torch.float64, device=gpu))
    with pytest.raises(TypeError, match="one dtype"):
        bu._group_grad(dict(shape=(B, c, N, m, s), idx=gi, dtype=torch.float16), torch.zeros((B, c, m, s), device=gpu))
    with pytest.raises(TypeError, match="one dtype"):
        ext.group_points_wrapper(B, c, N, m, s, f.half(), gi, torch.zeros((B, c, m, s), device=gpu))
    # coordinates are float32 only
    xyz = torch.rand((B, N, 3), device=gpu)
    for dtype in DTYPES + [torch.float64]:
        with pytest.raises(TypeError, match="float32 coordinates only"):
            bu.furthest_point_sample(xyz.to(dtype), 4)
        with pytest.raises(TypeError, match="float32 coordinates only"):
            bu.three_nn(xyz.to(dtype), xyz)
        with pytest.raises(TypeError, match="float32 coordinates only"):
            bu.three_nn(xyz, xyz.to(dtype))
        with pytest.raises(TypeError, match="float32 coordinates only"):
            bu.ball_query(1.0, 4, xyz.to(dtype), xyz)
        with pytest.raises(TypeError, match="float32 coordinates only"):
            bu.ball_query(1.0, 4, xyz, xyz.to(dtype))
    # the pools have no 16-bit form
    boxes = torch.tensor([[[2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 0.0]]], device=gpu).repeat(B, 1, 1)
    pf = torch.zeros((B, N, c), device=gpu)
    for dtype in DTYPES:
        with pytest.raises(TypeError, match="metres"):
            RoIPointPool3d(num_sampled_points=8)(xyz, pf.to(dtype), boxes)
        with pytest.raises(TypeError, match="float32 only"):
            RoIAwarePool3d(out_size=2, max_pts_each_voxel=4)(boxes[0], xyz[0].contiguous(), pf[0].to(dtype).contiguous())


def test_float32_still_goes_to_the_fp32_entry_points(gpu):
    """Integer values: the atomic forms' sums are exact in any order."""
    rng = np.random.default_rng(9)
    c, (m, s), n = 8, GROUP_SHAPES[0], QUERIES[1]
    gi, ai = _i(_fwd_idx(3, m * s, False).reshape(B, m, s), gpu), _i(_fwd_idx(4, GATHER_M[1], False), gpu)
    ii = _i(_fwd_idx(5, 3 * n, False).reshape(B, n, 3), gpu)
    w = _w(rng.choice(WEIGHTS, size=(B, n, 3)), gpu)
    f0 = _w(rng.integers(-8, 9, size=(B, c, N)), gpu)
    cases = [("fv2p_group_points_batch", (B, c, N, m, s), (B, c, N, m, s), lambda f: bu.grouping_operation(f, gi), [gi]),
             ("fv2p_gather_points", (B, c, N, GATHER_M[1]), (B, c, N, GATHER_M[1]), lambda f: bu.gather_operation(f, ai), [ai]),
             ("fv2p_three_interpolate_batch", (B, c, N, n), (B, c, n, N), lambda f: bu.three_interpolate(f, ii, w), [ii, w])]
    for det in (False, True):
        for name, fwd_sizes, bwd_sizes, apply, lists in cases:
            nat.set_deterministic(det)
            try:
                f = f0.clone().requires_grad_(True)
                out = apply(f)
                g = _w(rng.integers(-8, 9, size=tuple(out.shape)), gpu)
                out.backward(g)
            finally:
                nat.set_deterministic(False)
            assert out.dtype == f.grad.dtype == torch.float32
            ref = torch.empty_like(out)
            nat.call(name, *fwd_sizes, f0, *lists, ref, nat.stream())
            assert torch.equal(out, ref)
            dg = torch.zeros_like(f0)
            if det:
                ws = nat.workspace(getattr(nat.lib(), name + "_grad_ws_bytes")(*bwd_sizes), gpu)
                nat.call(name + "_grad_gather", *bwd_sizes, g, *lists, dg, ws, ws.numel(), nat.stream())
            else:
                nat.call(name + "_grad", *bwd_sizes, g, *lists, dg, nat.stream())
            assert torch.equal(f.grad, dg), name


# ---- the ext-module wrappers -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_ext_wrappers_take_16_bit_tensors(gpu, dtype):
    rng = np.random.default_rng(13)
    c, (m, s), n = 5, GROUP_SHAPES[0], QUERIES[1]
    gi, ai = _i(_fwd_idx(6, m * s, False).reshape(B, m, s), gpu), _i(_fwd_idx(7, GATHER_M[1], False), gpu)
    ii = _i(_fwd_idx(8, 3 * n, False).reshape(B, n, 3), gpu)
    w = _w(rng.random((B, n, 3)), gpu)
    cases = [(ext.group_points_wrapper, ext.group_points_grad_wrapper, (B, c, N, m, s), (B, c, N, m, s), [gi], lambda f: bu.grouping_operation(f, gi)),
             (ext.gather_points_wrapper, ext.gather_points_grad_wrapper, (B, c, N, GATHER_M[1]), (B, c, N, GATHER_M[1]), [ai],
              lambda f: bu.gather_operation(f, ai)),
             (ext.three_interpolate_wrapper, ext.three_interpolate_grad_wrapper, (B, c, N, n), (B, c, n, N), [ii, w],
              lambda f: bu.three_interpolate(f, ii, w))]
    for fwd, bwd, fwd_sizes, bwd_sizes, lists, apply in cases:
        f = _t(rng.standard_normal((B, c, N)), dtype, gpu).requires_grad_(True)
        out = apply(f)
        g = _t(rng.standard_normal(tuple(out.shape)), dtype, gpu)
        out.backward(g)
        mine = torch.full_like(out, float("nan"))
        assert fwd(*fwd_sizes, f.detach(), *lists, mine) == 1 and np.array_equal(bits(mine), bits(out))
        start = _t(rng.integers(-4, 5, size=(B, c, N)), dtype, gpu)
        for det in (False, True):                                           # the caller's buffer is accumulated into, once
            nat.set_deterministic(det)
            try:
                buf = start.clone()
                assert bwd(*bwd_sizes, g, *lists, buf) == 1
            finally:
                nat.set_deterministic(False)
            assert bool((f.grad != 0).any()) and np.array_equal(bits(buf), bits(start + f.grad))
        with pytest.raises(TypeError, match="one dtype"):
            fwd(*fwd_sizes, f.detach(), *lists, torch.empty(tuple(out.shape), device=gpu))
        with pytest.raises(TypeError, match="one dtype"):
            bwd(*bwd_sizes, g, *lists, torch.zeros((B, c, N), device=gpu))
