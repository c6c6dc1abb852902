"""GPU: the sparse group and the stacked grouping / interpolation on float16 / bfloat16 rows (csrc/sparse_aux.hip, csrc/pointnet2.hip,
the 16-bit form of csrc/scatter_add.hip), through the Python ops, the ext-module wrappers and the raw entry points.

  copies (grouping forward, indice_group forward): bit-equal to the fp32 op on the widened input, rounded back;
  interpolation forward: integer features in [-8, 8] with weights from {0, 1/4, 1/2, 1} are exact; random inputs satisfy
      |out - ref64| <= 2^-(p+1) |ref64| + 4 * 2^-24 * sum |w_i| |f_i| + 2^-25      (p = 10 fp16, 7 bf16; ref64 from the widened inputs):
      one final rounding, plus three products and two sums in fp32 (each within 2^-24 of a magnitude below the sum of the terms);
  gradients (fixed order, fp32 sums, one rounding): a row of k entries is within 2^-(p+1) |ref64| + (k + 2) 2^-24 sum |terms|
      (k products and fewer than k sums, whatever the association), exact on integer inputs, 0 on rows without entries in a
      NaN-filled output, entries outside the range dropped, two streams bit-identical;
  float64 raises TypeError; float32 keeps going to the fp32 entry points, bit for bit."""
import numpy as np
import pytest
import torch

import fv2p_native as nat
from exit_half_util import DT_CODE, DTYPES, PREC, bits, dtype_id, f64, missing_symbols, round_to
from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils as pu
from pcdet.ops.spconv import ops

pytestmark = pytest.mark.gpu
CHANNELS = [8, 5, 64]
S = 16
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


# ---- geometry shared by the tests (built once, never changed) ---------------------------------------------------------------
def _group_case():
    """Two samples: 25 + 15 feature rows, 9 + 6 key points, S = 16: 240 entries (no multiple of 32).  Global row 0 is the hub (100
    entries, four segments), global row 28 has exactly 32, rows 5, 6, 24 and 39 none, one entry of sample 1 points past the batch;
    key point 2 is an empty ball as ball_query leaves it (all samples row 0)."""
    rng = np.random.default_rng(11)
    fc, ic = np.array([25, 15], np.int32), np.array([9, 6], np.int32)
    a = np.concatenate([np.zeros(100 - S, np.int64), rng.choice([1, 2, 3, 4] + list(range(7, 24)), size=9 * S - S - (100 - S))])
    rng.shuffle(a)
    a = np.concatenate([a[:2 * S], np.zeros(S, np.int64), a[2 * S:]])          # key point 2: the empty ball, 16 more entries of the hub
    b = np.concatenate([np.full(32, 3, np.int64), [20], rng.choice([0, 1, 2] + list(range(4, 14)), size=6 * S - 33)])
    rng.shuffle(b)
    idx = np.concatenate([a, b]).reshape(15, S).astype(np.int32)
    glob = np.concatenate([a, b + 25])
    return dict(fc=fc, ic=ic, idx=idx, glob=glob, n=40, m=15)


def _interp_case():
    """77 queries (231 entries, no multiple of 32) into 40 known rows: row 0 the hub (100 entries), row 1 exactly 32, rows 5, 6 and 39
    none, one entry out of range."""
    rng = np.random.default_rng(12)
    flat = np.concatenate([np.zeros(100, np.int64), np.ones(32, np.int64), [43], rng.choice([2, 3, 4] + list(range(7, 39)), size=231 - 133)])
    rng.shuffle(flat)
    return dict(idx=flat.reshape(77, 3).astype(np.int32), n=77, m=40)


GROUP, INTERP = _group_case(), _interp_case()


def test_the_fixtures_hold_what_the_checks_need():
    for glob, n in ((GROUP["glob"], GROUP["n"]), (INTERP["idx"].reshape(-1), INTERP["m"])):
        cnt = np.bincount(glob[glob < n], minlength=n)
        assert cnt[0] == 100 and 32 in cnt[1:].tolist() and (cnt == 0).sum() >= 3 and (glob >= n).sum() == 1 and glob.size % 32 != 0
    assert (GROUP["idx"][2] == 0).all()


def _scatter_ref(dst, n_rows, coef, src64):
    """float64 reference of a scatter-add, the sum of |terms| and the entry count per row; entries outside [0, n_rows) are dropped."""
    keep = (dst >= 0) & (dst < n_rows)
    terms = coef[keep, None] * src64[keep]
    ref, mag = np.zeros((n_rows, src64.shape[1])), np.zeros((n_rows, src64.shape[1]))
    np.add.at(ref, dst[keep], terms)
    np.add.at(mag, dst[keep], np.abs(terms))
    return ref, mag, np.bincount(dst[keep], minlength=n_rows).astype(np.float64)[:, None]


def _check_rows(got, ref, mag, k, dtype, what):
    bound = 2.0 ** -(PREC[dtype] + 1) * np.abs(ref) + (k + 2) * EPS24 * mag
    err = np.abs(got - ref)
    print("%s: max err / bound = %.3f" % (what, (err / np.maximum(bound, 1e-300)).max()))
    assert np.isfinite(got).all() and (err <= bound).all(), what


# ---- copies ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_grouping_forward_is_a_copy(gpu, dtype, c):
    f = _t(np.random.default_rng(c).standard_normal((GROUP["n"], c)), dtype, gpu)
    idx = _i(np.minimum(GROUP["idx"], GROUP["fc"].repeat(GROUP["ic"])[:, None] - 1), gpu)        # the forward reads every row it is given
    fc, ic = _i(GROUP["fc"], gpu), _i(GROUP["ic"], gpu)
    out = pu.grouping_operation(f, fc, idx, ic)
    ref = pu.grouping_operation(f.float(), fc, idx, ic).to(dtype)
    assert out.dtype == dtype and out.shape == (GROUP["m"], c, S)
    assert np.array_equal(bits(out), bits(ref))
    # a row outside the batch gives zeros (raw entry point; the fp32 kernel would read it)
    raw = torch.full((GROUP["m"], c, S), float("nan"), dtype=dtype, device=gpu)
    nat.call("fv2p_group_points_stack_h", 2, GROUP["m"], c, GROUP["n"], S, f, fc, _i(GROUP["idx"], gpu), ic, raw, DT_CODE[dtype], nat.stream())
    far = torch.from_numpy(GROUP["glob"].reshape(-1, S) >= GROUP["n"]).to(gpu)
    assert int(far.sum()) == 1
    keep = ~far[:, None, :].expand(-1, c, -1)
    assert torch.equal(raw[keep].view(torch.int16), out[keep].view(torch.int16)) and bool((raw[~keep] == 0).all())


def _strided_book(gpu, seed, rows=120, shape=(7, 10, 9)):
    rng = np.random.default_rng(seed)
    flat = np.sort(rng.choice(2 * int(np.prod(shape)), size=rows, replace=False))
    ind = _i(np.stack(np.unravel_index(flat, (2,) + shape), 1), gpu)
    book = ops.build_rulebook(ind, 2, list(shape), [3, 3, 3], [2, 2, 2], [1, 1, 1], [1, 1, 1], 0, False)
    return book, rows, int(book.outids.shape[0])


@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_indice_group_forward_is_a_copy_and_backward_rounds_once(gpu, dtype, c):
    book, n_in, n_out = _strided_book(gpu, 5)
    rng = np.random.default_rng(100 + c)
    f = _t(rng.standard_normal((n_in, c)), dtype, gpu)
    out = ops.indice_group(f, book, None, n_out)
    ref = ops.indice_group(f.float(), book, None, n_out)
    assert out.dtype == dtype and out.shape == (27, n_out, c) and bool((ref == 0).any())
    assert np.array_equal(bits(out), bits(ref.to(dtype)))
    # backward: fp32 sum over ascending k, one rounding: k = kvol terms
    tab, flip = book.in_table()
    tab = (tab.flip(0) if flip else tab).long().cpu().numpy()                        # [27, n_in] -> output row or -1
    for exact in (True, False):
        g64 = rng.integers(-8, 9, size=(27, n_out, c)).astype(np.float64) if exact else round_to(rng.standard_normal((27, n_out, c)), dtype)
        din = ops.indice_group_backward(f, _t(g64, dtype, gpu), book, None)
        assert din.dtype == dtype and din.shape == (n_in, c)
        picked = np.where(tab[:, :, None] >= 0, g64[np.arange(27)[:, None], np.maximum(tab, 0)], 0.0)      # [27, n_in, c]
        ref64, mag = picked.sum(0), np.abs(picked).sum(0)
        if exact:
            assert np.array_equal(f64(din), round_to(ref64, dtype))
        else:
            _check_rows(f64(din), ref64, mag, 27.0, dtype, "indice_group_backward")
    with pytest.raises(TypeError, match="one dtype"):
        ops.indice_group_backward(f, torch.zeros((27, n_out, c), device=gpu), book, None)


# ---- interpolation forward -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_interpolation_forward(gpu, dtype, c):
    rng = np.random.default_rng(200 + c)
    n, m = 300, 50
    idx = rng.integers(0, m, size=(n, 3)).astype(np.int32)
    for exact in (True, False):
        f64_ = rng.integers(-8, 9, size=(m, c)).astype(np.float64) if exact else round_to(rng.standard_normal((m, c)), dtype)
        w = rng.choice(WEIGHTS, size=(n, 3)) if exact else rng.random((n, 3)).astype(np.float32).astype(np.float64)
        out = pu.three_interpolate(_t(f64_, dtype, gpu), _i(idx, gpu), torch.from_numpy(w.astype(np.float32)).to(gpu))
        assert out.dtype == dtype and out.shape == (n, c)
        terms = w[:, :, None] * f64_[idx]                                              # [n, 3, c]
        ref64, mag = terms.sum(1), np.abs(terms).sum(1)
        if exact:
            assert np.array_equal(f64(out), round_to(ref64, dtype))
        else:
            bound = 2.0 ** -(PREC[dtype] + 1) * np.abs(ref64) + 4 * EPS24 * mag + 2.0 ** -25
            err = np.abs(f64(out) - ref64)
            print("three_interpolate: max err / bound = %.3f" % (err / bound).max())
            assert (err <= bound).all()


# ---- gradients ----------------------------------------------------------------------------------------------------------------------
def _interp_grad_raw(g, idx, w, m, dtype, gpu):
    n, c = g.shape
    out = torch.full((m, c), float("nan"), dtype=dtype, device=gpu)
    ws = nat.workspace(nat.lib().fv2p_three_interpolate_stack_grad_h_ws_bytes(n, c, m), gpu)
    nat.call("fv2p_three_interpolate_stack_grad_h", n, c, m, g, idx, w, out, DT_CODE[dtype], ws, ws.numel(), nat.stream())
    return out


def _group_grad_raw(g, idx, ic, fc, n, dtype, gpu):
    m, c, s = g.shape
    out = torch.full((n, c), float("nan"), dtype=dtype, device=gpu)
    ws = nat.workspace(nat.lib().fv2p_group_points_stack_grad_h_ws_bytes(m, c, s), gpu)
    nat.call("fv2p_group_points_stack_grad_h", ic.numel(), m, c, n, s, g, idx, ic, fc, out, DT_CODE[dtype], ws, ws.numel(), nat.stream())
    return out


def _on_two_streams(fn):
    outs = []
    for _ in range(2):
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            outs.append(fn())
        st.synchronize()
    return outs


@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_interpolation_gradient(gpu, dtype, c):
    rng = np.random.default_rng(300 + c)
    n, m, idx_np = INTERP["n"], INTERP["m"], INTERP["idx"]
    idx = _i(idx_np, gpu)
    for exact in (True, False):
        g64 = rng.integers(-8, 9, size=(n, c)).astype(np.float64) if exact else round_to(rng.standard_normal((n, c)), dtype)
        w64 = rng.choice(WEIGHTS, size=(n, 3)) if exact else rng.random((n, 3)).astype(np.float32).astype(np.float64)
        g, w = _t(g64, dtype, gpu), torch.from_numpy(w64.astype(np.float32)).to(gpu)
        a, b = _on_two_streams(lambda: _interp_grad_raw(g, idx, w, m, dtype, gpu))
        assert np.array_equal(bits(a), bits(b))
        ref64, mag, k = _scatter_ref(idx_np.reshape(-1).astype(np.int64), m, w64.reshape(-1), np.repeat(g64, 3, axis=0))
        got = f64(a)
        assert (got[(k == 0)[:, 0]] == 0).all() and (k == 0).sum() >= 3
        if exact:
            assert np.abs(ref64).max() < 2048 and np.array_equal(got, round_to(ref64, dtype))
        else:
            _check_rows(got, ref64, mag, k, dtype, "three_interpolate gradient")
        # the autograd route reaches the same entry point, whatever the switches say
        feats = torch.zeros((m, c), dtype=dtype, device=gpu, requires_grad=True)
        safe = _i(np.minimum(idx_np, m - 1), gpu)                                      # the forward reads every row it is given
        for det in (False, True):
            nat.set_deterministic(det)
            try:
                feats.grad = None
                pu.three_interpolate(feats, safe, w).backward(g)
            finally:
                nat.set_deterministic(False)
            assert feats.grad.dtype == dtype
            assert np.array_equal(bits(feats.grad), bits(_interp_grad_raw(g, safe, w, m, dtype, gpu)))


@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_grouping_gradient(gpu, dtype, c):
    rng = np.random.default_rng(400 + c)
    n, m = GROUP["n"], GROUP["m"]
    idx, fc, ic = _i(GROUP["idx"], gpu), _i(GROUP["fc"], gpu), _i(GROUP["ic"], gpu)
    for exact in (True, False):
        g64 = rng.integers(-8, 9, size=(m, c, S)).astype(np.float64) if exact else round_to(rng.standard_normal((m, c, S)), dtype)
        g = _t(g64, dtype, gpu)
        a, b = _on_two_streams(lambda: _group_grad_raw(g, idx, ic, fc, n, dtype, gpu))
        assert np.array_equal(bits(a), bits(b))
        src = g64.transpose(0, 2, 1).reshape(m * S, c)                                 # entry (point, sample) -> its C gradients
        ref64, mag, k = _scatter_ref(GROUP["glob"], n, np.ones(m * S), src)
        got = f64(a)
        assert (got[(k == 0)[:, 0]] == 0).all() and (k == 0).sum() >= 3
        if exact:
            assert np.abs(ref64).max() < 2048 and np.array_equal(got, round_to(ref64, dtype))
        else:
            _check_rows(got, ref64, mag, k, dtype, "grouping gradient")
        feats = torch.zeros((n, c), dtype=dtype, device=gpu, requires_grad=True)
        safe = _i(np.minimum(GROUP["idx"], GROUP["fc"].repeat(GROUP["ic"])[:, None] - 1), gpu)
        for det in (False, True):
            nat.set_deterministic(det)
            try:
                feats.grad = None
                pu.grouping_operation(feats, fc, safe, ic).backward(g)
            finally:
                nat.set_deterministic(False)
            assert feats.grad.dtype == dtype
            assert np.array_equal(bits(feats.grad), bits(_group_grad_raw(g, safe, ic, fc, n, dtype, gpu)))


# ---- the ext-module wrappers -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [8, 5])                                        # the 16-byte path and the element path
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_ext_wrappers_take_16_bit_tensors(gpu, dtype, c):
    """pointnet2_stack_cuda on 16-bit buffers: the forward wrappers fill the caller's buffer with the bits of the Python ops, the gradient
    wrappers accumulate the autograd route's gradient into it once, switch off and on; source and destination of two dtypes raise."""
    from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_stack_cuda as ext
    rng = np.random.default_rng(500 + c)
    n, m = GROUP["n"], GROUP["m"]
    gidx, fc, ic, iidx = _i(GROUP["idx"], gpu), _i(GROUP["fc"], gpu), _i(GROUP["ic"], gpu), _i(INTERP["idx"], gpu)
    w = torch.from_numpy(rng.random((INTERP["n"], 3)).astype(np.float32)).to(gpu)
    cases = [(n, lambda f: pu.grouping_operation(f, fc, gidx, ic), lambda f, out: ext.group_points_wrapper(2, m, c, S, f, fc, gidx, ic, out),
              lambda g, buf: ext.group_points_grad_wrapper(2, m, c, n, S, g, gidx, ic, fc, buf)),
             (INTERP["m"], lambda f: pu.three_interpolate(f, iidx, w), lambda f, out: ext.three_interpolate_wrapper(f, iidx, w, out),
              lambda g, buf: ext.three_interpolate_grad_wrapper(g, iidx, w, buf))]
    for rows, apply, fwd, bwd in cases:
        f = _t(rng.standard_normal((rows, c)), dtype, gpu).requires_grad_(True)
        out = apply(f)
        g = _t(rng.standard_normal(tuple(out.shape)), dtype, gpu)
        out.backward(g)
        mine = torch.full_like(out, float("nan"))
        assert fwd(f.detach(), mine) == 1 and np.array_equal(bits(mine), bits(out))
        start = _t(rng.integers(-4, 5, size=(rows, c)), dtype, gpu)
        for det in (False, True):                                           # the caller's buffer is accumulated into, once
            nat.set_deterministic(det)
            try:
                buf = start.clone()
                assert bwd(g, buf) == 1
            finally:
                nat.set_deterministic(False)
            assert bool((f.grad != 0).any()) and np.array_equal(bits(buf), bits(start + f.grad))
        with pytest.raises(TypeError, match="one dtype"):
            fwd(f.detach(), torch.empty(tuple(out.shape), device=gpu))
        with pytest.raises(TypeError, match="one dtype"):
            bwd(g, torch.zeros((rows, c), device=gpu))


# ---- dtypes that are not served, and float32 left alone ---------------------------------------------------------------------------------
def test_float64_raises_and_float32_still_goes_to_the_fp32_entry_points(gpu):
    rng = np.random.default_rng(9)
    c, n, m = 8, GROUP["n"], GROUP["m"]
    fc, ic = _i(GROUP["fc"], gpu), _i(GROUP["ic"], gpu)
    gidx = _i(np.minimum(GROUP["idx"], GROUP["fc"].repeat(GROUP["ic"])[:, None] - 1), gpu)
    iidx = _i(np.minimum(INTERP["idx"], INTERP["m"] - 1), gpu)
    w = torch.from_numpy(rng.choice(WEIGHTS, size=(INTERP["n"], 3)).astype(np.float32)).to(gpu)
    f_g = torch.from_numpy(rng.integers(-8, 9, size=(n, c)).astype(np.float32)).to(gpu)
    f_i = torch.from_numpy(rng.integers(-8, 9, size=(INTERP["m"], c)).astype(np.float32)).to(gpu)
    with pytest.raises(TypeError, match="float32, float16 and bfloat16"):
        pu.grouping_operation(f_g.double(), fc, gidx, ic)
    with pytest.raises(TypeError, match="float32, float16 and bfloat16"):
        pu.three_interpolate(f_i.double(), iidx, w)
    with pytest.raises(TypeError, match="float32, float16 and bfloat16"):
        pu._group_grad(dict(dims=(2, m, c, n, S), idx=gidx, ic=ic, fc=fc), torch.zeros((m, c, S), dtype=torch.float64, device=gpu))
    with pytest.raises(TypeError, match="float32, float16 and bfloat16"):
        pu._interp_grad(dict(idx=iidx, weight=w, rows=INTERP["m"]), torch.zeros((INTERP["n"], c), dtype=torch.float64, device=gpu))
    # float32: the same bits as the fp32 entry points called directly (integer values: the atomic forms' sums are exact in any order)
    for det in (False, True):
        nat.set_deterministic(det)
        try:
            fg, fi = f_g.clone().requires_grad_(True), f_i.clone().requires_grad_(True)
            og, oi = pu.grouping_operation(fg, fc, gidx, ic), pu.three_interpolate(fi, iidx, w)
            gg = torch.from_numpy(rng.integers(-8, 9, size=tuple(og.shape)).astype(np.float32)).to(gpu)
            gi = torch.from_numpy(rng.integers(-8, 9, size=tuple(oi.shape)).astype(np.float32)).to(gpu)
            og.backward(gg)
            oi.backward(gi)
        finally:
            nat.set_deterministic(False)
        assert og.dtype == oi.dtype == fg.grad.dtype == fi.grad.dtype == torch.float32
        rg, ri = torch.empty_like(og), torch.empty_like(oi)
        nat.call("fv2p_group_points_stack", 2, m, c, S, f_g, fc, gidx, ic, rg, nat.stream())
        nat.call("fv2p_three_interpolate_stack", INTERP["n"], c, f_i, iidx, w, ri, nat.stream())
        assert torch.equal(og, rg) and torch.equal(oi, ri)
        dg, di = torch.zeros_like(f_g), torch.zeros_like(f_i)
        if det:
            ws = nat.workspace(nat.lib().fv2p_group_points_stack_grad_ws_bytes(m, c, S), gpu)
            nat.call("fv2p_group_points_stack_grad_gather", 2, m, c, n, S, gg, gidx, ic, fc, dg, ws, ws.numel(), nat.stream())
            ws = nat.workspace(nat.lib().fv2p_three_interpolate_stack_grad_ws_bytes(INTERP["n"], c, INTERP["m"]), gpu)
            nat.call("fv2p_three_interpolate_stack_grad_gather", INTERP["n"], c, INTERP["m"], gi, iidx, w, di, ws, ws.numel(), nat.stream())
        else:
            nat.call("fv2p_group_points_stack_grad", 2, m, c, n, S, gg, gidx, ic, fc, dg, nat.stream())
            nat.call("fv2p_three_interpolate_stack_grad", INTERP["n"], c, gi, iidx, w, di, nat.stream())
        assert torch.equal(fg.grad, dg) and torch.equal(fi.grad, di)
