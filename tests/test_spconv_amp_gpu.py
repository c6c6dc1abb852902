"""GPU: the sparse convolution in mixed precision - float32 master weights and bias beside float16 / bfloat16 features and gradients
(fv2p_sparse_conv_rows_hw32 / fv2p_sparse_conv_wgrad_hw32 of csrc/sparse_conv_h.hip, spconv.set_mixed_precision).  Geometry, operands and
oracle results come from half_cases.py; the fp32 weights and biases from amp_cases.py.

  1. exact cases ({-1, 0, 1} operands): forward, d features, the fp32 d weight and the fp32 d bias equal the oracle bit for bit;
  2. in-kernel rounding: fp32 weights that are no values of the 16-bit dtype (ties, float16 subnormals, -0.0 among them) give the BITS of
     the uniform 16-bit route on weight.to(dtype) - output, d features, and d weight after .to(dtype);
  3. the fp32 d weight against float64: |got - ref| <= e + 2^-24, e = n_pairs 2^-24 S (the bound of test_spconv_half_gpu.py with u = 0:
     this result is not rounded to 16 bits), through the raw entry point and through the modules;
  4. an fp32 bias that is no value of the dtype: |got - ref64| <= u (|ref64| + e) + e + 2^-24 with |bias| added to S and one more term;
  5. the raw row entry point with transpose_w / flip_k 0 and 1, unknown dtypes, n_dst = 0, a workspace that is too small;
  6. the switch and the autocast rules;  7. a conv / BatchNorm / ReLU / max-pool / dense() chain under autocast against the uniform
  16-bit stack, bit for bit;  8. torch.amp.GradScaler;  9. run-to-run bit identity;  10. an empty input;  11. the modules' cached
  16-bit copy of the weights (ops.cached_copy_pays) follows an optimiser step, and test 2 also holds functions against modules.
Every test restores the switch in a `finally`."""
import copy

import numpy as np
import pytest
import torch
from torch import nn

import amp_cases
import fv2p_native as nat
import half_cases
import oracle
import pcdet.ops.spconv as spconv
from pcdet.ops.spconv import ops

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]
DT_CODE = {torch.float16: 1, torch.bfloat16: 2}
UNIT = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
dtype_id = lambda d: str(d).replace("torch.", "")


def _dev(a, dtype, gpu):
    """Host array -> device tensor of `dtype` (through float32)."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(gpu).to(dtype)


def _host(t):
    return t.detach().float().cpu()


def _bits(t):
    return t.detach().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _build(case, gpu, feats_dtype):
    """The case's conv module with float32 parameters (not yet on the GPU) and its input tensor with features of `feats_dtype`."""
    kind, cin, cout, batch, shape = case["kind"], case["cin"], case["cout"], case["batch"], case["shape"]
    ind = torch.from_numpy(case["ind"]).to(gpu)
    feats = _dev(case["feats"], feats_dtype, gpu).requires_grad_(True)
    if kind == "subm":
        conv = spconv.SubMConv3d(cin, cout, 3, padding=1, bias=False, indice_key="k")
        x = spconv.SparseConvTensor(feats, ind, shape, batch)
    elif kind == "strided":
        conv = spconv.SparseConv3d(cin, cout, 3, stride=2, padding=1, bias=case["bias"] is not None, indice_key="d")
        x = spconv.SparseConvTensor(feats, ind, shape, batch)
    else:   # the inverse conv reads the rulebook its strided partner left under the same key
        down = spconv.SparseConv3d(8, 8, 3, stride=2, padding=1, bias=False, indice_key="d").to(gpu).to(feats_dtype)
        with torch.no_grad():
            x = down(spconv.SparseConvTensor(torch.zeros((ind.shape[0], 8), dtype=feats_dtype, device=gpu), ind, shape, batch))
        assert np.array_equal(x.indices.cpu().numpy(), case["outids"])
        x.features = feats
        conv = spconv.SparseInverseConv3d(cin, cout, 3, indice_key="d", bias=False)
    return conv, x, feats


def run(case, dtype, gpu, mixed, w=None, bias=None):
    """Forward and backward of the case's conv through the module API with 16-bit features and output gradient.  mixed: the module
    keeps float32 parameters (the switch is on in the caller); otherwise it is converted with .to(dtype): the uniform 16-bit route.
    `w` / `bias`: float32 host arrays that replace the case's.  -> (out, d features, d weight, d bias or None, module, input tensor)."""
    conv, x, feats = _build(case, gpu, dtype)
    conv = conv.to(gpu)
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(np.array(case["w"] if w is None else w, np.float32)))
        b = case["bias"] if bias is None else bias
        if conv.bias is not None:
            conv.bias.copy_(torch.from_numpy(np.array(b, np.float32)))
    if not mixed:
        conv = conv.to(dtype)
    y = conv(x)
    assert y.features.dtype == dtype and tuple(y.features.shape) == case["ref"].shape
    y.features.backward(_dev(case["g"], dtype, gpu))
    pdt = torch.float32 if mixed else dtype
    assert feats.grad.dtype == dtype and conv.weight.grad.dtype == pdt
    assert conv.bias is None or conv.bias.grad.dtype == pdt
    return y.features, feats.grad, conv.weight.grad, None if conv.bias is None else conv.bias.grad, conv, x


def run_functions(case, dtype, gpu, w):
    """The case through ops.indice_conv / ops.indice_conv_backward with float32 weights: no module, hence no cached 16-bit copy of the
    weights - every row conv is the `hw32` kernel.  -> (out, d features, d weight)"""
    subm = case["kind"] == "subm"
    ind = torch.from_numpy(case["ind"]).to(gpu)
    rb = ops.build_rulebook(ind, case["batch"], case["shape"], 3, 1 if subm else 2, 1, 1, 0, subm)
    assert subm or np.array_equal(rb.outids.cpu().numpy(), case["outids"])
    feats, g, w32 = _dev(case["feats"], dtype, gpu), _dev(case["g"], dtype, gpu), torch.from_numpy(np.array(w, np.float32)).to(gpu)
    out = ops.indice_conv(feats, w32, rb, None, case["n_dst"], False, subm)
    din, dw = ops.indice_conv_backward(feats, w32, g, rb, None, False, subm)
    return out, din, dw


def assert_exact(case, dtype, gpu):
    spconv.set_mixed_precision(True)
    try:
        out, din, dw, db, conv, x = run(case, dtype, gpu, mixed=True)
        assert torch.equal(_host(out), torch.from_numpy(case["ref"])), "forward"
        assert torch.equal(_host(din), torch.from_numpy(case["din"])), "input gradient"
        assert dw.dtype == torch.float32 and torch.equal(dw.cpu(), torch.from_numpy(case["dw"])), "weight gradient"
        if case["bias"] is not None:
            assert db.dtype == torch.float32 and torch.equal(db.cpu(), torch.from_numpy(case["g"].sum(0))), "bias gradient"
            conv.fused_bn = True   # the folded inference conv of SparseSequential.fused(): the same kernel call
            with torch.no_grad():
                fused = conv(spconv.SparseConvTensor(x.features.detach(), x.indices, x.spatial_shape, x.batch_size))
            assert fused.features.dtype == dtype and torch.equal(_host(fused.features), torch.from_numpy(case["ref"])), "fused bias"
    finally:
        spconv.set_mixed_precision(False)


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


@pytest.mark.parametrize("cin,cout", half_cases.CHANNELS)
@pytest.mark.parametrize("kind", ["subm", "strided"])
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_weights_rounded_in_the_kernel_give_the_bits_of_the_uniform_route(gpu, dtype, kind, cin, cout):
    case = half_cases.random_case(kind, cin, cout, dtype)
    w = amp_cases.weights(cin, cout, dtype)
    uni = run(case, dtype, gpu, mixed=False, w=w)
    spconv.set_mixed_precision(True)
    try:
        mix = run(case, dtype, gpu, mixed=True, w=w)
        fun = run_functions(case, dtype, gpu, w)
    finally:
        spconv.set_mixed_precision(False)
    for t in mix[:3] + uni[:3]:
        assert bool(torch.isfinite(t).all())
    # the functions (always the `hw32` kernels) and the modules (a cached 16-bit copy where ops.cached_copy_pays says so): the same bits
    assert fun[0].dtype == dtype and fun[1].dtype == dtype and fun[2].dtype == torch.float32
    for name, a, b in zip(("forward", "input gradient", "weight gradient"), fun, mix[:3]):
        assert torch.equal(_bits(a), _bits(b)), "functions against modules: " + name
    assert torch.equal(_bits(mix[0]), _bits(uni[0])), "forward"
    assert torch.equal(_bits(mix[1]), _bits(uni[1])), "input gradient"
    assert mix[2].dtype == torch.float32 and uni[2].dtype == dtype
    assert torch.equal(_bits(mix[2].to(dtype)), _bits(uni[2])), "weight gradient"
    # the master weights were read, not replaced: still the float32 values, none of them a value of the dtype
    assert torch.equal(mix[4].weight.detach().cpu(), torch.from_numpy(np.array(w)))


def _assert_dw_within(got, case, what):
    """|got - ref| <= e + 2^-24, e = n_pairs 2^-24 S, element-wise (u = 0: no rounding to 16 bits); prints the largest ratio first."""
    assert got.dtype == torch.float32
    got = got.detach().cpu().double().numpy().reshape(case["dw"].shape)
    n_dw = case["n_dw"].reshape(3, 3, 3, 1, 1).astype(np.float64)
    bound = n_dw * 2.0 ** -24 * case["s_dw"] + 2.0 ** -24
    ratio = np.abs(got - case["dw"]) / bound
    print("%s: max |err| / bound = %.3f (max |err| %.3e, max |ref| %.3e)" % (what, ratio.max(), np.abs(got - case["dw"]).max(), np.abs(case["dw"]).max()))
    assert np.isfinite(got).all() and ratio.max() <= 1.0, what


@pytest.mark.parametrize("cin,cout", amp_cases.WGRAD_CHANNELS)
@pytest.mark.parametrize("kind", ["subm", "strided"])
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_fp32_weight_gradient_within_the_derived_bound(gpu, dtype, kind, cin, cout):
    case = half_cases.random_case(kind, cin, cout, dtype)
    n_dst = case["n_dst"]
    src, g = _dev(case["feats"], dtype, gpu), _dev(case["g"], dtype, gpu)
    tab = torch.from_numpy(amp_cases.tables(case)).to(gpu)
    ws = nat.workspace(nat.lib().fv2p_sparse_conv_wgrad_h_ws_bytes(n_dst, cin, cout, 27), gpu)
    dw = torch.full((27, cin, cout), 77.0, dtype=torch.float32, device=gpu)
    nat.call("fv2p_sparse_conv_wgrad_hw32", src, src.shape[0], cin, g, tab, n_dst, cout, 27, 0, dw, DT_CODE[dtype], ws, ws.numel(), nat.stream())
    _assert_dw_within(dw, case, "raw entry point")
    spconv.set_mixed_precision(True)
    try:
        dw_mod = run(case, dtype, gpu, mixed=True)[2]
    finally:
        spconv.set_mixed_precision(False)
    _assert_dw_within(dw_mod, case, "modules")
    assert torch.equal(_bits(dw_mod.reshape(27, cin, cout)), _bits(dw))   # the same launches either way


def _assert_within(got, ref, s, n_terms, u, what):
    """|got - ref| <= u (|ref| + e) + e + 2^-24 with e = n_terms 2^-24 s, element-wise (the form of test_spconv_half_gpu.py)."""
    got = _host(got).double().numpy()
    e = n_terms * 2.0 ** -24 * s
    bound = u * (np.abs(ref) + e) + e + 2.0 ** -24
    ratio = np.abs(got - ref) / bound
    print("%s: max |err| / bound = %.3f (max |err| %.3e, max |ref| %.3e)" % (what, ratio.max(), np.abs(got - ref).max(), np.abs(ref).max()))
    assert np.isfinite(got).all() and ratio.max() <= 1.0, what


@pytest.mark.parametrize("cin,cout", amp_cases.BIAS_CHANNELS)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_fp32_bias_joins_the_fp32_sum_unrounded(gpu, dtype, cin, cout):
    case = dict(half_cases.random_case("strided", cin, cout, dtype))
    b = amp_cases.bias(cout, dtype)
    case["bias"] = b
    spconv.set_mixed_precision(True)
    try:
        out, _, _, db, _, _ = run(case, dtype, gpu, mixed=True)
    finally:
        spconv.set_mixed_precision(False)
    b64 = b.astype(np.float64)
    _assert_within(out, case["ref"] + b64, case["s_ref"] + np.abs(b64), case["n_ref"] + 1, UNIT[dtype], "forward with fp32 bias")
    # d bias: the float32 column sum of the 16-bit output gradient (n_dst terms per column)
    g = case["g"]
    bound = g.shape[0] * 2.0 ** -24 * np.abs(g).sum(0) + 2.0 ** -24
    assert db.dtype == torch.float32 and (np.abs(db.cpu().double().numpy() - g.sum(0)) <= bound).all()


def _rows_hw32(src, w, tab, n_dst, c_dst, flip, transpose_w, bias, dtype_code, dst):
    return nat.lib().fv2p_sparse_conv_rows_hw32(src.data_ptr(), src.shape[0], src.shape[1], w.data_ptr(), tab.shape[0], tab.data_ptr(), n_dst, c_dst,
                                                flip, transpose_w, 0 if bias is None else bias.data_ptr(), dst.data_ptr(), dtype_code, nat.stream())


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_raw_entry_points_transpose_flip_bias_and_argument_checks(gpu, dtype):
    case = half_cases.exact_case("strided", 32, 64)
    cin, cout, n_dst = case["cin"], case["cout"], case["n_dst"]
    tab_np = amp_cases.tables(case)
    src, bias = _dev(case["feats"], dtype, gpu), _dev(case["bias"], torch.float32, gpu)
    w_np = case["w"].reshape(27, cin, cout)
    ref = torch.from_numpy(case["ref"])
    for transpose_w in (0, 1):
        for flip in (0, 1):
            # the same conv said four ways: W_k handed over as W_k^T [K][Cout][Cin] for transpose_w = 1; for flip_k = 1 the kernel reads
            # table row K-1-k with weight k, so it is given the table with its rows reversed
            wk = w_np.transpose(0, 2, 1) if transpose_w else w_np
            tab = torch.from_numpy(np.ascontiguousarray(tab_np[::-1] if flip else tab_np)).to(gpu)
            dst = torch.full((n_dst, cout), 77.0, dtype=dtype, device=gpu)
            rc = _rows_hw32(src, _dev(wk, torch.float32, gpu), tab, n_dst, cout, flip | (ops.TAB_PLANNED if transpose_w else 0), transpose_w, bias,
                            DT_CODE[dtype], dst)
            assert rc == 0, nat.last_error()
            assert torch.equal(_host(dst), ref), (transpose_w, flip)
    # unknown dtype: an error, and nothing is launched (dst keeps its fill)
    tab = torch.from_numpy(tab_np).to(gpu)
    w = _dev(w_np, torch.float32, gpu)
    dst = torch.full((n_dst, cout), 77.0, dtype=dtype, device=gpu)
    lib = nat.lib()
    need = lib.fv2p_sparse_conv_wgrad_h_ws_bytes(n_dst, cin, cout, 27)
    ws = nat.workspace(need, gpu)
    dw = torch.full((27, cin, cout), 77.0, dtype=torch.float32, device=gpu)
    g = _dev(case["g"], dtype, gpu)
    wgrad = lambda n, code, nbytes: lib.fv2p_sparse_conv_wgrad_hw32(src.data_ptr(), src.shape[0], cin, g.data_ptr(), tab.data_ptr(), n, cout, 27, 0,
                                                                    dw.data_ptr(), code, ws.data_ptr(), nbytes, nat.stream())
    for bad in (0, 3, -1):
        assert _rows_hw32(src, w, tab, n_dst, cout, 0, 0, bias, bad, dst) < 0
        assert "dtype" in nat.last_error()
        assert wgrad(n_dst, bad, ws.numel()) < 0
        assert "dtype" in nat.last_error()
    # a workspace that is too small is refused
    assert need > 16 and wgrad(n_dst, DT_CODE[dtype], need - 16) < 0
    assert "workspace" in nat.last_error()
    # n_dst = 0: success, nothing launched
    assert _rows_hw32(src, w, tab, 0, cout, 0, 0, bias, DT_CODE[dtype], dst) == 0
    assert wgrad(0, DT_CODE[dtype], ws.numel()) == 0
    torch.cuda.synchronize()
    assert bool((dst == 77.0).all()) and bool((dw == 77.0).all())
    # ... and the weight gradient entry point itself, on the forward table
    assert wgrad(n_dst, DT_CODE[dtype], ws.numel()) == 0, nat.last_error()
    assert torch.equal(dw.cpu(), torch.from_numpy(case["dw"].reshape(27, cin, cout)))


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_switch_and_autocast_rules(gpu, dtype):
    case = half_cases.exact_case("subm", 16, 16, 17, half_cases.EDGE_BATCH, tuple(half_cases.EDGE_SHAPE))
    ind = torch.from_numpy(case["ind"]).to(gpu)
    conv = spconv.SubMConv3d(16, 16, 3, padding=1, bias=True).to(gpu)   # float32 parameters
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(case["w"].copy()))
    tensor = lambda f: spconv.SparseConvTensor(f, ind, case["shape"], case["batch"])
    assert not spconv.mixed_precision()
    with pytest.raises(TypeError, match="one dtype"):
        conv(tensor(_dev(case["feats"], dtype, gpu)))
    with torch.autocast("cuda", dtype=dtype):
        with pytest.raises(TypeError, match="one dtype"):
            conv(tensor(_dev(case["feats"], dtype, gpu)))
    spconv.set_mixed_precision(True)
    try:
        feats = _dev(case["feats"], torch.float32, gpu).requires_grad_(True)
        with torch.autocast("cuda", dtype=dtype):
            y = conv(tensor(feats))
        assert y.features.dtype == dtype
        y.features.backward(_dev(case["g"], dtype, gpu))   # outside the autocast region, as a training loop's backward is
        assert feats.grad.dtype == torch.float32 and conv.weight.grad.dtype == torch.float32 and conv.bias.grad.dtype == torch.float32
        assert torch.equal(feats.grad.cpu(), torch.from_numpy(case["din"])) and torch.equal(conv.weight.grad.cpu(), torch.from_numpy(case["dw"]))
        # an output gradient of another dtype still raises
        rb = ops.build_rulebook(ind, case["batch"], case["shape"], 3, 1, 1, 1, 0, True)
        f16 = _dev(case["feats"], dtype, gpu)
        assert ops.indice_conv(f16, conv.weight.detach(), rb, None, 17, False, True).dtype == dtype
        with pytest.raises(TypeError, match="output gradient"):
            ops.indice_conv_backward(f16, conv.weight.detach(), _dev(case["g"], torch.float32, gpu), rb, None, False, True)
        # outside autocast float32 features and float32 weights stay on the float32 route
        conv.zero_grad()
        f32 = _dev(case["feats"], torch.float32, gpu).requires_grad_(True)
        y32 = conv(tensor(f32))
        assert y32.features.dtype == torch.float32
        y32.features.backward(_dev(case["g"], torch.float32, gpu))
        assert f32.grad.dtype == torch.float32 and conv.weight.grad.dtype == torch.float32
    finally:
        spconv.set_mixed_precision(False)


class _Probe(spconv.SparseModule):
    """Records the dtype of the features that pass."""

    def __init__(self, seen):
        super().__init__()
        self.seen = seen

    def forward(self, x):
        self.seen.append(x.features.dtype)
        return x


class _EpilogueBiasConv(torch.autograd.Function):
    """The uniform 16-bit submanifold conv with its bias added in the kernel's epilogue (ops.fused_indice_conv: one rounding of the
    output), with a backward.  The uniform MODULE adds the bias in a second pass over the rounded output - two roundings, other bits
    than the mixed route's one - so the comparison stack of the chain test calls the conv this way."""

    @staticmethod
    def forward(ctx, feats, w, b, rb):
        ctx.rb = rb
        ctx.save_for_backward(feats, w)
        return ops.fused_indice_conv(feats, w, b, rb, None, feats.shape[0], False, True)

    @staticmethod
    def backward(ctx, g):
        feats, w = ctx.saved_tensors
        din, dw = ops.indice_conv_backward(feats, w, g.contiguous(), ctx.rb, None, False, True)
        return din, dw, g.sum(0, dtype=torch.float32).to(g.dtype), None


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_chain_under_autocast_equals_the_uniform_16_bit_stack(gpu, dtype):
    geo = half_cases.geometry("subm", amp_cases.CHAIN_BATCH, tuple(amp_cases.CHAIN_SHAPE), amp_cases.CHAIN_ROWS, 4242)
    ind = torch.from_numpy(geo["ind"]).to(gpu)
    torch.manual_seed(11)
    bn = lambda c: nn.BatchNorm1d(c, eps=1e-3, momentum=0.01)
    seen = []
    mods = [spconv.SubMConv3d(16, 16, 3, padding=1, bias=False, indice_key="s1"), bn(16), nn.ReLU(),
            spconv.SparseConv3d(16, 32, 3, stride=2, padding=1, bias=False, indice_key="d2"), bn(32), nn.ReLU(),
            spconv.SubMConv3d(32, 32, 3, padding=1, bias=True, indice_key="s2"), bn(32), nn.ReLU()]
    with torch.no_grad():
        mods[6].bias.copy_(torch.randn(32).to(dtype).float())        # a value of the dtype: the uniform route holds it in 16 bits
        for m in mods:
            if isinstance(m, nn.BatchNorm1d):
                m.weight.copy_(torch.rand(m.num_features) + 0.5)
                m.bias.copy_(torch.randn(m.num_features) * 0.1)
    pool = spconv.SparseMaxPool3d(3, stride=2, padding=1)
    ref_mods = copy.deepcopy(mods)
    net = spconv.SparseSequential(mods[0], mods[1], mods[2], _Probe(seen), mods[3], mods[4], mods[5], _Probe(seen), mods[6], mods[7], mods[8],
                                  _Probe(seen), pool, _Probe(seen)).to(gpu).train()
    feats32 = torch.randn(ind.shape[0], 16, device=gpu)
    # ---- the comparison: convs .to(dtype), BatchNorm parameters float32, features cast by hand, no autocast, switch off
    ref_mods = [m.to(gpu) for m in ref_mods]
    for i in (0, 3, 6):
        ref_mods[i] = ref_mods[i].to(dtype)
    head = spconv.SparseSequential(*ref_mods[:6]).train()
    tail = spconv.SparseSequential(ref_mods[7], ref_mods[8]).train()
    fr = feats32.to(dtype).requires_grad_(True)
    h = head(spconv.SparseConvTensor(fr, ind, amp_cases.CHAIN_SHAPE, amp_cases.CHAIN_BATCH))
    rb3 = ops.build_rulebook(h.indices, amp_cases.CHAIN_BATCH, h.spatial_shape, 3, 1, 1, 1, 0, True)
    h.features = _EpilogueBiasConv.apply(h.features, ref_mods[6].weight, ref_mods[6].bias, rb3)
    dense_ref = pool(tail(h)).dense()
    assert dense_ref.dtype == dtype
    g = torch.randn(dense_ref.shape, device=gpu).to(dtype)
    dense_ref.backward(g)
    # ---- the mixed stack: float32 parameters, float32 input features, autocast, switch on
    spconv.set_mixed_precision(True)
    try:
        fm = feats32.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=dtype):
            dense = net(spconv.SparseConvTensor(fm, ind, amp_cases.CHAIN_SHAPE, amp_cases.CHAIN_BATCH)).dense()
        dense.backward(g)
    finally:
        spconv.set_mixed_precision(False)
    assert dense.dtype == dtype and seen == [dtype] * 4, seen
    assert torch.equal(_bits(dense), _bits(dense_ref)), "dense maps"
    assert fm.grad.dtype == torch.float32 and torch.equal(_bits(fm.grad.to(dtype)), _bits(fr.grad)), "input gradient"
    for i, (m, r) in enumerate(zip(mods, ref_mods)):
        if isinstance(m, nn.BatchNorm1d):
            for name in ("weight", "bias"):
                a, b = getattr(m, name).grad, getattr(r, name).grad
                assert a.dtype == torch.float32 and torch.equal(_bits(a), _bits(b)), (i, name)
            assert torch.equal(_bits(m.running_mean), _bits(r.running_mean)) and torch.equal(_bits(m.running_var), _bits(r.running_var)), i
            assert int(m.num_batches_tracked) == int(r.num_batches_tracked) == 1
        elif isinstance(m, spconv.SparseConvolution):
            assert m.weight.dtype == torch.float32 and m.weight.grad.dtype == torch.float32 and r.weight.grad.dtype == dtype
            assert bool(torch.isfinite(m.weight.grad).all()) and bool((m.weight.grad != 0).any())
            assert torch.equal(_bits(m.weight.grad.to(dtype)), _bits(r.weight.grad)), (i, "weight gradient")
            if m.bias is not None:
                assert m.bias.grad.dtype == torch.float32 and torch.equal(_bits(m.bias.grad.to(dtype)), _bits(r.bias.grad)), (i, "bias gradient")


def test_grad_scaler_float16(gpu):
    dtype = torch.float16
    case = half_cases.random_case("subm", 16, 16, dtype)
    ind = torch.from_numpy(case["ind"]).to(gpu)
    torch.manual_seed(5)
    conv = spconv.SubMConv3d(16, 16, 3, padding=1, bias=False, indice_key="k").to(gpu)
    block = spconv.SparseSequential(nn.BatchNorm1d(16, eps=1e-3, momentum=0.01), nn.ReLU()).to(gpu).train()
    params = [conv.weight] + list(block.parameters())
    opt = torch.optim.SGD(params, lr=0.1)
    scaler = torch.amp.GradScaler("cuda", init_scale=16.0)
    feats32 = _dev(case["feats"], torch.float32, gpu)
    grads = []

    def forward():
        with torch.autocast("cuda", dtype=dtype):
            y = conv(spconv.SparseConvTensor(feats32, ind, case["shape"], case["batch"]))
            y.features.register_hook(lambda g: grads.append(g.detach().clone()))
            out = block(y)
            assert y.features.dtype == dtype and out.features.dtype == dtype
            return out.features, out.features.float().square().sum()

    spconv.set_mixed_precision(True)
    try:
        forward()[1].backward()                                   # the unscaled run
        dw_plain, g_plain = conv.weight.grad.clone(), grads.pop()
        assert dw_plain.dtype == torch.float32 and g_plain.dtype == dtype
        opt.zero_grad(set_to_none=True)
        scaler.scale(forward()[1]).backward()
        scaler.unscale_(opt)                                      # raises for float16 parameter gradients; these are float32
        dw_scaled = conv.weight.grad.clone()
        # both are fp32 sums of the same products, one of them of gradients scaled by 16 and divided again: the bound of test 3, with S
        # and the pair counts from the operands the GPU used
        _, s_dw = oracle.indice_conv_backward(np.abs(case["feats"]), np.abs(conv.weight.detach().cpu().double().numpy()),
                                              g_plain.cpu().double().abs().numpy(), case["pairs"], case["num"], subm=True)
        n_dw = np.asarray(case["num"], np.float64).reshape(3, 3, 3, 1, 1)
        bound = n_dw * 2.0 ** -24 * s_dw.numpy() + 2.0 ** -24
        err = (dw_scaled.double() - dw_plain.double()).abs().cpu().numpy()
        print("unscaled against plain: max |err| / bound = %.3f" % (err / bound).max())
        assert np.isfinite(err).all() and (err <= bound).all()
        scaler.step(opt)
        scaler.update()
        assert scaler.get_scale() == 16.0
        # an overflow: one inf in the output gradient -> a non-finite float32 d weight -> the step is skipped, the scale halved
        opt.zero_grad(set_to_none=True)
        before = [p.detach().clone() for p in params]
        out, loss = forward()
        g = torch.ones_like(out)
        g.view(-1)[out.detach().argmax()] = float("inf")            # where the ReLU is open: the overflow reaches the conv
        scaler.scale(loss)
        out.backward(g)
        assert conv.weight.grad.dtype == torch.float32 and not bool(torch.isfinite(conv.weight.grad).all())
        scaler.step(opt)
        scaler.update()
        assert scaler.get_scale() == 8.0
        for p, q in zip(params, before):
            assert torch.equal(p.detach(), q)
    finally:
        spconv.set_mixed_precision(False)


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_two_runs_are_bit_identical(gpu, dtype):
    case = half_cases.random_case("subm", 64, 128, dtype)
    w = amp_cases.weights(64, 128, dtype)
    spconv.set_mixed_precision(True)
    try:
        a = run(case, dtype, gpu, mixed=True, w=w)[:3]
        b = run(case, dtype, gpu, mixed=True, w=w)[:3]
    finally:
        spconv.set_mixed_precision(False)
    assert a[2].dtype == torch.float32
    for p, q in zip(a, b):
        assert torch.equal(_bits(p), _bits(q))


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_the_cached_16_bit_copy_follows_the_master_weights(gpu, dtype):
    """A module whose shape takes the cached 16-bit copy (ops.cached_copy_pays): after an in-place update of the float32 weight - an
    optimiser step - the next pass uses the new values."""
    case = half_cases.random_case("subm", 32, 32, dtype)
    assert ops.cached_copy_pays(32, 32, None) and not ops.cached_copy_pays(32, 32, torch.zeros(32)) and not ops.cached_copy_pays(3, 7, None)
    conv, x, feats = _build(case, gpu, dtype)
    conv = conv.to(gpu)
    opt = torch.optim.SGD(conv.parameters(), lr=0.5)
    g = _dev(case["g"], dtype, gpu)
    spconv.set_mixed_precision(True)
    try:
        conv(x).features.backward(g)
        first = conv._weight16(dtype)
        assert conv._weight16(dtype) is first and torch.equal(_bits(first), _bits(conv.weight.detach().to(dtype)))
        opt.step()
        y = conv(x).features
        assert conv._weight16(dtype) is not first and torch.equal(_bits(conv._weight16(dtype)), _bits(conv.weight.detach().to(dtype)))
    finally:
        spconv.set_mixed_precision(False)
    ref = copy.deepcopy(conv).to(dtype)(spconv.SparseConvTensor(x.features.detach(), x.indices, x.spatial_shape, x.batch_size)).features
    assert torch.equal(_bits(y), _bits(ref)) and not torch.equal(_bits(first), _bits(conv.weight.detach().to(dtype)))


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_empty_input_gives_an_empty_output_of_the_16_bit_dtype(gpu, dtype):
    conv = spconv.SubMConv3d(16, 32, 3, padding=1, bias=True).to(gpu)
    x = spconv.SparseConvTensor(torch.zeros((0, 16), dtype=dtype, device=gpu), torch.zeros((0, 4), dtype=torch.int32, device=gpu), [4, 4, 4], 1)
    spconv.set_mixed_precision(True)
    try:
        y = conv(x)
    finally:
        spconv.set_mixed_precision(False)
    assert tuple(y.features.shape) == (0, 32) and y.features.dtype == dtype
