"""GPU: the fused sparse convolution on float16 / bfloat16 tensors (csrc/sparse_conv_h.hip) through the pcdet.ops.spconv modules and the
raw C ABI.  Cases and oracle results come from half_cases.py.

  1. exact cases ({-1, 0, 1} operands): forward, input gradient and weight gradient equal the oracle bit for bit;
  2. random cases: |got - ref64| <= u (|ref64| + e) + e + 2^-24 element-wise, with nothing measured in the bound:
       u = 2^-11 (float16) / 2^-8 (bfloat16): ONE rounding of the result to 16 bits;
       e = n_terms 2^-24 S: the worst case of summing n_terms fp32 terms of absolute sum S in any order (the 16-bit products are
           exact in fp32); n_terms = kvol * gathered channels for the row convs, the pair count of offset k for dW_k;
       2^-24: float16 results below 2^-14 are subnormal and round with an absolute, not a relative, error;
  3. the raw entry point with transpose_w / flip_k 0 and 1, an unknown dtype, n_dst = 0;
  4. no fp32 copy of an operand: the peak memory of a forward + backward stays below the size of the upcast copies alone;
  5. two runs are bit-identical;  6. an empty tensor gives a [0, cout] result of the input's dtype."""
import numpy as np
import pytest
import torch

import fv2p_native as nat
import half_cases
import pcdet.ops.spconv as spconv
from pcdet.ops.spconv import ops

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]
DT_CODE = {torch.float16: 1, torch.bfloat16: 2}
UNIT = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
dtype_id = lambda d: str(d).replace("torch.", "")


def _dev(a, dtype, gpu):
    """Host array (values representable in `dtype`) -> device tensor of that dtype."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(gpu).to(dtype)


def _host(t):
    return t.detach().float().cpu()


def run_modules(case, dtype, gpu):
    """Forward and backward of the case's conv through the module API -> (out, d features, d weight, module, input tensor)."""
    kind, cin, cout, batch, shape = case["kind"], case["cin"], case["cout"], case["batch"], case["shape"]
    ind = torch.from_numpy(case["ind"]).to(gpu)
    feats = _dev(case["feats"], dtype, gpu).requires_grad_(True)
    if kind == "subm":
        conv = spconv.SubMConv3d(cin, cout, 3, padding=1, bias=False, indice_key="k")
        x = spconv.SparseConvTensor(feats, ind, shape, batch)
    elif kind == "strided":
        conv = spconv.SparseConv3d(cin, cout, 3, stride=2, padding=1, bias=case["bias"] is not None, indice_key="d")
        x = spconv.SparseConvTensor(feats, ind, shape, batch)
    else:   # the inverse conv reads the rulebook its strided partner left under the same key
        down = spconv.SparseConv3d(8, 8, 3, stride=2, padding=1, bias=False, indice_key="d").to(gpu).to(dtype)
        with torch.no_grad():
            x = down(spconv.SparseConvTensor(torch.zeros((ind.shape[0], 8), dtype=dtype, device=gpu), ind, shape, batch))
        assert np.array_equal(x.indices.cpu().numpy(), case["outids"])
        x.features = feats
        conv = spconv.SparseInverseConv3d(cin, cout, 3, indice_key="d", bias=False)
    conv = conv.to(gpu).to(dtype)
    with torch.no_grad():
        conv.weight.copy_(_dev(case["w"], dtype, gpu))
        if conv.bias is not None:
            conv.bias.copy_(_dev(case["bias"], dtype, gpu))
    y = conv(x)
    assert y.features.dtype == dtype and tuple(y.features.shape) == case["ref"].shape
    if kind == "strided":
        assert np.array_equal(y.indices.cpu().numpy(), case["outids"])
    y.features.backward(_dev(case["g"], dtype, gpu))
    assert feats.grad.dtype == dtype and conv.weight.grad.dtype == dtype
    return y.features, feats.grad, conv.weight.grad, conv, x


def assert_exact(case, dtype, gpu):
    out, din, dw, conv, x = run_modules(case, dtype, gpu)
    assert torch.equal(_host(out), torch.from_numpy(case["ref"])), "forward"
    assert torch.equal(_host(din), torch.from_numpy(case["din"])), "input gradient"
    assert torch.equal(_host(dw), torch.from_numpy(case["dw"])), "weight gradient"
    if case["bias"] is not None:   # the same conv with the bias added in the kernel's epilogue (fused_bn modules, inference)
        assert torch.equal(_host(conv.bias.grad), torch.from_numpy(case["g"].sum(0)))
        conv.fused_bn = True
        with torch.no_grad():
            fused = conv(spconv.SparseConvTensor(x.features.detach(), x.indices, x.spatial_shape, x.batch_size))
        assert fused.features.dtype == dtype and torch.equal(_host(fused.features), torch.from_numpy(case["ref"])), "fused bias"


@pytest.mark.parametrize("cin,cout", half_cases.CHANNELS)
@pytest.mark.parametrize("kind", half_cases.KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_exact_cases_equal_the_oracle_bit_for_bit(gpu, dtype, kind, cin, cout):
    assert_exact(half_cases.exact_case(kind, cin, cout), dtype, gpu)


@pytest.mark.parametrize("rows", half_cases.EDGE_ROWS)
@pytest.mark.parametrize("cin,cout", half_cases.EDGE_CHANNELS)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_exact_cases_at_wave_group_and_tile_edges(gpu, dtype, cin, cout, rows):
    case = half_cases.exact_case("subm", cin, cout, rows, half_cases.EDGE_BATCH, tuple(half_cases.EDGE_SHAPE))
    assert case["n_dst"] == rows
    assert_exact(case, dtype, gpu)


def _assert_within(got, ref, s, n_terms, u, what):
    """|got - ref| <= u (|ref| + e) + e + 2^-24 with e = n_terms 2^-24 s, element-wise; prints the largest ratio before it asserts."""
    got = _host(got).double().numpy()
    e = n_terms * 2.0 ** -24 * s
    bound = u * (np.abs(ref) + e) + e + 2.0 ** -24
    ratio = np.abs(got - ref) / bound
    print("%s: max |err| / bound = %.3f (max |err| %.3e, max |ref| %.3e)" % (what, ratio.max(), np.abs(got - ref).max(), np.abs(ref).max()))
    assert np.isfinite(got).all() and ratio.max() <= 1.0, what


@pytest.mark.parametrize("cin,cout", half_cases.CHANNELS)
@pytest.mark.parametrize("kind", ["subm", "strided"])
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_random_cases_within_the_derived_bound(gpu, dtype, kind, cin, cout):
    case = half_cases.random_case(kind, cin, cout, dtype)
    out, din, dw, _, _ = run_modules(case, dtype, gpu)
    u = UNIT[dtype]
    _assert_within(out, case["ref"], case["s_ref"], case["n_ref"], u, "forward")
    _assert_within(din, case["din"], case["s_din"], case["n_din"], u, "input gradient")
    n_dw = case["n_dw"].reshape(3, 3, 3, 1, 1).astype(np.float64)
    _assert_within(dw, case["dw"], case["s_dw"], n_dw, u, "weight gradient")


def _tables(case, gpu):
    """tab_out [K, n_dst] of the case's rulebook from the oracle's pair lists: the source row of destination row o at offset k, or -1."""
    pairs, num = case["pairs"], case["num"]
    tab = np.full((pairs.shape[0], case["n_dst"]), -1, np.int32)
    for k in range(pairs.shape[0]):
        tab[k, pairs[k, 1, :num[k]]] = pairs[k, 0, :num[k]]
    return tab


def _rows_h(src, w, tab, n_dst, c_dst, flip, transpose_w, bias, dtype_code, dst):
    return nat.lib().fv2p_sparse_conv_rows_h(src.data_ptr(), src.shape[0], src.shape[1], w.data_ptr(), tab.shape[0], tab.data_ptr(), n_dst, c_dst,
                                             flip, transpose_w, 0 if bias is None else bias.data_ptr(), dst.data_ptr(), dtype_code, nat.stream())


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_raw_entry_point_transpose_flip_bias_and_argument_checks(gpu, dtype):
    case = half_cases.exact_case("strided", 32, 64)
    cin, cout, n_dst = case["cin"], case["cout"], case["n_dst"]
    tab_np = _tables(case, gpu)
    src, bias = _dev(case["feats"], dtype, gpu), _dev(case["bias"], dtype, gpu)
    w_np = case["w"].reshape(27, cin, cout)
    ref = torch.from_numpy(case["ref"])
    for transpose_w in (0, 1):
        for flip in (0, 1):
            # the same conv said four ways: W_k handed over as W_k^T [K][Cout][Cin] for transpose_w = 1; for flip_k = 1 the kernel reads
            # table row K-1-k with weight k, so it is given the table with its rows reversed
            wk = w_np.transpose(0, 2, 1) if transpose_w else w_np
            tab = torch.from_numpy(np.ascontiguousarray(tab_np[::-1] if flip else tab_np)).to(gpu)
            dst = torch.full((n_dst, cout), 77.0, dtype=dtype, device=gpu)
            rc = _rows_h(src, _dev(wk, dtype, gpu), tab, n_dst, cout, flip | (ops.TAB_PLANNED if transpose_w else 0), transpose_w, bias, DT_CODE[dtype], dst)
            assert rc == 0, nat.last_error()
            assert torch.equal(_host(dst), ref), (transpose_w, flip)
    # unknown dtype: an error, and nothing is launched (dst keeps its fill)
    tab = torch.from_numpy(tab_np).to(gpu)
    dst = torch.full((n_dst, cout), 77.0, dtype=dtype, device=gpu)
    for bad in (0, 3, -1):
        assert _rows_h(src, _dev(w_np, dtype, gpu), tab, n_dst, cout, 0, 0, bias, bad, dst) < 0
        assert "dtype" in nat.last_error()
    lib = nat.lib()
    ws = nat.workspace(lib.fv2p_sparse_conv_wgrad_h_ws_bytes(n_dst, cin, cout, 27), gpu)
    dw = torch.full((27, cin, cout), 77.0, dtype=dtype, device=gpu)
    g = _dev(case["g"], dtype, gpu)
    assert lib.fv2p_sparse_conv_wgrad_h(src.data_ptr(), src.shape[0], cin, g.data_ptr(), tab.data_ptr(), n_dst, cout, 27, 0, dw.data_ptr(), 9,
                                        ws.data_ptr(), ws.numel(), nat.stream()) < 0
    # n_dst = 0: success, nothing launched
    assert _rows_h(src, _dev(w_np, dtype, gpu), tab, 0, cout, 0, 0, bias, DT_CODE[dtype], dst) == 0
    assert lib.fv2p_sparse_conv_wgrad_h(src.data_ptr(), src.shape[0], cin, g.data_ptr(), tab.data_ptr(), 0, cout, 27, 0, dw.data_ptr(), DT_CODE[dtype],
                                        ws.data_ptr(), ws.numel(), nat.stream()) == 0
    torch.cuda.synchronize()
    assert bool((dst == 77.0).all()) and bool((dw == 77.0).all())
    # ... and the weight gradient entry point itself, on the forward table
    nat.call("fv2p_sparse_conv_wgrad_h", src, src.shape[0], cin, g, tab, n_dst, cout, 27, 0, dw, DT_CODE[dtype], ws, ws.numel(), nat.stream())
    assert torch.equal(_host(dw), torch.from_numpy(case["dw"].reshape(27, cin, cout)))


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_mixed_and_unsupported_dtypes_raise(gpu, dtype):
    case = half_cases.exact_case("subm", 16, 16, 17, half_cases.EDGE_BATCH, tuple(half_cases.EDGE_SHAPE))
    ind = torch.from_numpy(case["ind"]).to(gpu)
    conv = spconv.SubMConv3d(16, 16, 3, padding=1, bias=False).to(gpu)   # float32 weights
    with pytest.raises(TypeError, match="one dtype"):
        conv(spconv.SparseConvTensor(_dev(case["feats"], dtype, gpu), ind, case["shape"], case["batch"]))
    with pytest.raises(NotImplementedError, match="float32, float16 and bfloat16"):
        conv.double()(spconv.SparseConvTensor(_dev(case["feats"], torch.float64, gpu), ind, case["shape"], case["batch"]))


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_no_fp32_copy_of_an_operand_is_made(gpu, dtype):
    """A route through the fp32 kernels has to hold fp32 copies of the features (4 n cin bytes), of the output gradient (4 n cout) and
    of the weights (4 K cin cout) at the same time in its backward, before any result is allocated.  The native route allocates only
    16-bit results (out, d features, d weight: 2 bytes per element): its peak stays below the size of those copies alone."""
    case = half_cases.random_case("subm", 64, 64, dtype)
    n, cin, cout = case["n_dst"], 64, 64
    conv = spconv.SubMConv3d(cin, cout, 3, padding=1, bias=False, indice_key="k").to(gpu).to(dtype)
    feats, g = _dev(case["feats"], dtype, gpu).requires_grad_(True), _dev(case["g"], dtype, gpu)
    x = spconv.SparseConvTensor(feats, torch.from_numpy(case["ind"]).to(gpu), case["shape"], case["batch"])
    conv(x).features.backward(g)   # rulebook (kept on x), grow-only workspace and gradient buffers exist from here on
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    conv(x).features.backward(g)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    upcast_copies = 4 * (n * cin + n * cout + 27 * cin * cout)
    native_results = 2 * (n * cout + n * cin + 27 * cin * cout)
    print("peak %d bytes; 16-bit results %d; fp32 copies of the operands %d" % (peak, native_results, upcast_copies))
    assert peak < upcast_copies


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_two_runs_are_bit_identical(gpu, dtype):
    case = half_cases.random_case("subm", 64, 128, dtype)
    a = run_modules(case, dtype, gpu)[:3]
    b = run_modules(case, dtype, gpu)[:3]
    for p, q in zip(a, b):
        assert torch.equal(p.view(torch.int16), q.view(torch.int16))


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_empty_input_gives_an_empty_output_of_the_same_dtype(gpu, dtype):
    conv = spconv.SubMConv3d(16, 32, 3, padding=1, bias=False).to(gpu).to(dtype)
    x = spconv.SparseConvTensor(torch.zeros((0, 16), dtype=dtype, device=gpu), torch.zeros((0, 4), dtype=torch.int32, device=gpu), [4, 4, 4], 1)
    y = conv(x)
    assert tuple(y.features.shape) == (0, 32) and y.features.dtype == dtype
