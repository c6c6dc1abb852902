"""GPU: the sparse max-pool on float16 / bfloat16 rows (fv2p_sparse_maxpool_fwd_h / _bwd_h, csrc/sparse_aux.hip) through
SparseMaxPool3d(3, 2, 1) and the raw entry points, against oracle.indice_maxpool(+_backward) on the rounded inputs.

  forward : max(0, max_k in) compared on the widened values - one of the inputs or 0, so bit-equal to the oracle, in the input's dtype;
  backward: din = sum_k [in == out] dout - bit-equal for ternary dout (sums of at most 27 integers), within one rounding u |ref| of
            the oracle's sum for random dout (the oracle adds the same fp32 terms over ascending k);
  inputs are rounded normals (half of them negative: the clamp at 0 shows) with every row duplicated, so that ties occur;
  no fp32 copy: the peak of forward + backward stays below 4 (n_in + 2 n_out) c bytes;  two runs are bit-identical."""
import numpy as np
import pytest
import torch

import fv2p_native as nat
import half_cases
import oracle
import pcdet.ops.spconv as spconv
from pcdet.ops.spconv import functional as Fsp
from pcdet.ops.spconv import ops

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]
DT_CODE = {torch.float16: 1, torch.bfloat16: 2}
UNIT = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
dtype_id = lambda d: str(d).replace("torch.", "")
BATCH, SHAPE = 2, [9, 20, 18]
ROWS, CHANNELS = [1, 17, 900], [8, 16, 20, 7, 128]


def _dev(a, dtype, gpu):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(gpu).to(dtype)


def _host(t):
    return t.detach().float().cpu().numpy()


def make_case(rows, c, dtype):
    geo = half_cases.geometry("strided", BATCH, tuple(SHAPE), rows, 4000 + 10 * rows + c)
    rng = np.random.default_rng(rows * 131 + c)
    n_in, n_out = geo["n_src"], geo["n_dst"]
    base = half_cases.round_to(rng.standard_normal(((n_in + 1) // 2, c)), dtype).astype(np.float32)
    feats = np.concatenate([base, base])[rng.permutation(2 * base.shape[0])[:n_in]]     # every value occurs twice: ties
    ref = oracle.indice_maxpool(feats, geo["pairs"], geo["num"], n_out)
    tern = (rng.integers(-1, 2, size=(n_out, c))).astype(np.float32)
    rand = half_cases.round_to(rng.standard_normal((n_out, c)), dtype).astype(np.float32)
    return dict(geo, feats=feats, ref=ref, tern=tern, rand=rand, n_in=n_in, n_out=n_out,
                din_tern=oracle.indice_maxpool_backward(feats, ref, tern, geo["pairs"], geo["num"]),
                din_rand=oracle.indice_maxpool_backward(feats, ref, rand, geo["pairs"], geo["num"]))


def _tables(case):
    pairs, num = case["pairs"], case["num"]
    tab_out = np.full((pairs.shape[0], case["n_out"]), -1, np.int32)
    tab_in = np.full((pairs.shape[0], case["n_in"]), -1, np.int32)
    for k in range(pairs.shape[0]):
        tab_out[k, pairs[k, 1, :num[k]]] = pairs[k, 0, :num[k]]
        tab_in[k, pairs[k, 0, :num[k]]] = pairs[k, 1, :num[k]]
    return tab_in, tab_out


@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_module_and_raw_entry_points_against_the_oracle(gpu, dtype, rows, c):
    case = make_case(rows, c, dtype)
    u = UNIT[dtype]
    assert (case["feats"] < 0).mean() > 0.3 and (case["ref"] >= 0).all()
    ind = torch.from_numpy(case["ind"]).to(gpu)
    pool = spconv.SparseMaxPool3d(3, 2, 1)
    for gname, dname, exact in (("tern", "din_tern", True), ("rand", "din_rand", False)):
        feats = _dev(case["feats"], dtype, gpu).requires_grad_(True)
        y = pool(spconv.SparseConvTensor(feats, ind, SHAPE, BATCH))
        assert np.array_equal(y.indices.cpu().numpy(), case["outids"])
        assert y.features.dtype == dtype
        assert np.array_equal(_host(y.features), case["ref"])
        y.features.backward(_dev(case[gname], dtype, gpu))
        assert feats.grad.dtype == dtype
        got, ref = _host(feats.grad).astype(np.float64), case[dname].astype(np.float64)
        if exact:
            assert np.abs(ref).max() <= 27 and np.array_equal(got, ref)
        else:
            print("din: max |err| / (u |ref|) = %.3f" % (np.abs(got - ref) / np.maximum(u * np.abs(ref), 1e-300)).max())
            assert (np.abs(got - ref) <= u * np.abs(ref)).all()
    # raw entry points on tables built from the oracle's pair lists; flip_k = 1 reads table row K-1-k (a max does not care)
    tab_in_np, tab_out_np = _tables(case)
    f, g = _dev(case["feats"], dtype, gpu), _dev(case["tern"], dtype, gpu)
    lib = nat.lib()
    for flip in (0, 1):
        tab_out = torch.from_numpy(np.ascontiguousarray(tab_out_np[::-1] if flip else tab_out_np)).to(gpu)
        out = torch.full((case["n_out"], c), 77.0, dtype=dtype, device=gpu)
        nat.call("fv2p_sparse_maxpool_fwd_h", f, case["n_in"], c, tab_out, 27, case["n_out"], flip, out, DT_CODE[dtype], nat.stream())
        assert np.array_equal(_host(out), case["ref"]), flip
    tab_in = torch.from_numpy(tab_in_np).to(gpu)
    din = torch.full((case["n_in"], c), 77.0, dtype=dtype, device=gpu)
    for bad in (0, 3, -1):   # unknown dtype: an error, nothing launched
        assert lib.fv2p_sparse_maxpool_fwd_h(f.data_ptr(), case["n_in"], c, tab_out.data_ptr(), 27, case["n_out"], 0, din.data_ptr(), bad, nat.stream()) < 0
        assert "dtype" in nat.last_error()
        assert lib.fv2p_sparse_maxpool_bwd_h(f.data_ptr(), out.data_ptr(), g.data_ptr(), case["n_in"], c, tab_in.data_ptr(), 27, din.data_ptr(), bad,
                                             nat.stream()) < 0
        assert "dtype" in nat.last_error()
    assert lib.fv2p_sparse_maxpool_bwd_h(f.data_ptr(), out.data_ptr(), g.data_ptr(), 0, c, tab_in.data_ptr(), 27, din.data_ptr(), DT_CODE[dtype], nat.stream()) == 0
    torch.cuda.synchronize()
    assert bool((din == 77.0).all())
    nat.call("fv2p_sparse_maxpool_bwd_h", f, out, g, case["n_in"], c, tab_in, 27, din, DT_CODE[dtype], nat.stream())
    assert np.array_equal(_host(din), case["din_tern"])


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_mixed_and_unsupported_dtypes_raise(gpu, dtype):
    case = make_case(17, 8, dtype)
    tab_in_np, tab_out_np = _tables(case)
    tab_in, tab_out = torch.from_numpy(tab_in_np).to(gpu), torch.from_numpy(tab_out_np).to(gpu)
    f = _dev(case["feats"], dtype, gpu)
    out = ops._table_maxpool(f, tab_out, False, case["n_out"])
    assert out.dtype == dtype
    with pytest.raises(TypeError, match="one dtype"):
        ops._table_maxpool_backward(f, out, torch.ones_like(out, dtype=torch.float32), tab_in)
    with pytest.raises(NotImplementedError, match="float32, float16 and bfloat16"):
        ops._table_maxpool(f.double(), tab_out, False, case["n_out"])


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_no_fp32_copy_and_two_runs_bit_identical(gpu, dtype):
    """fp32 copies of in, out and dout are 4 (n_in + 2 n_out) c bytes; the native route allocates the 16-bit out and din only."""
    c = 128
    case = make_case(900, c, dtype)
    n_in, n_out = case["n_in"], case["n_out"]
    book = ops.build_rulebook(torch.from_numpy(case["ind"]).to(gpu), BATCH, SHAPE, [3, 3, 3], [2, 2, 2], [1, 1, 1], [1, 1, 1], 0, False)
    feats, g = _dev(case["feats"], dtype, gpu).requires_grad_(True), _dev(case["rand"], dtype, gpu)

    def step():
        y = Fsp.indice_maxpool(feats, book, None, n_out)
        y.backward(g)
        din, feats.grad = feats.grad, None
        return y.detach(), din

    a = step()   # both tables of the rulebook exist from here on
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    b = step()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print("peak %d bytes; 16-bit results %d; fp32 copies %d" % (peak, 2 * (n_in + n_out) * c, 4 * (n_in + 2 * n_out) * c))
    assert peak < 4 * (n_in + 2 * n_out) * c
    for p, q in zip(a, b):
        assert p.dtype == dtype and torch.equal(p.view(torch.int16), q.view(torch.int16))
