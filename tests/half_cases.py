"""Cases of the 16-bit sparse conv tests (test_spconv_half_cpu.py, test_spconv_half_gpu.py).  Host only: geometry, operands and the
oracle's results; every case is built once per process and read by all tests that use it.

EXACT cases: features and output gradients in {-1, 0, 1} (non-zero with probability 1/4), weights in {-1, 0, 1}, bias in {-2 .. 2}.
Every product and every partial sum is a small integer, exact in fp32 in any summation order, so a kernel that stores 16 bits must
reproduce the oracle BIT FOR BIT as long as the results themselves are representable: integers up to 256 are exact in bfloat16
(8 significant bits), up to 2048 in float16.  `exact_case` asserts max|ref| <= 256 for the forward result and both gradients; the
condition is a property of the inputs (checked without a GPU by test_spconv_half_cpu.py) and the seeds below satisfy it.

RANDOM cases: standard-normal operands ROUNDED TO THE CASE'S DTYPE FIRST, the reference computed in float64 from the rounded values
(the oracle works in float64 when handed float64), and the same oracle run on the absolute values, which gives S = sum |terms| per
output element - the scale of the fp32 accumulation error bound the GPU test derives."""
import functools

import numpy as np
import torch

import oracle
from sparse_util import random_active

CHANNELS = [(16, 16), (32, 32), (32, 64), (64, 64), (64, 128), (128, 128), (24, 40), (3, 7), (5, 16), (160, 144)]
KINDS = ("subm", "strided", "inverse")
BATCH, SHAPE, ROWS = 2, [9, 20, 18], 900
EDGE_CHANNELS = [(32, 32), (64, 64)]
EDGE_ROWS = [1, 15, 16, 17, 63, 64, 65]       # wave-group (16) and tile edges; rows with no neighbour but themselves
EDGE_BATCH, EDGE_SHAPE = 2, [5, 12, 12]
EXACT_MAX = 256                                # bfloat16 represents every integer up to 2^8
K3, ONE3, TWO3 = [3, 3, 3], [1, 1, 1], [2, 2, 2]


def _seed(kind, cin, cout, rows):
    return 1000 * KINDS.index(kind) + 100 * cin + cout + 7 * rows


@functools.lru_cache(maxsize=None)
def geometry(kind, batch, shape, rows, seed):
    """Active set and the oracle's rulebook.  -> dict(ind, outids, pairs, num, n_src, n_dst): the conv of `kind` gathers n_src rows and
    writes n_dst rows (inverse: from the strided conv's outputs back to its inputs)."""
    shape = list(shape)
    ind = random_active(seed, batch, shape, rows)
    if kind == "subm":
        outids, pairs, num = oracle.indice_pairs(ind, batch, shape, K3, ONE3, ONE3, ONE3, subm=True)
        n_src = n_dst = ind.shape[0]
    else:
        outids, pairs, num = oracle.indice_pairs(ind, batch, shape, K3, TWO3, ONE3, ONE3)
        n_src, n_dst = (outids.shape[0], ind.shape[0]) if kind == "inverse" else (ind.shape[0], outids.shape[0])
    return dict(ind=ind, outids=outids, pairs=pairs, num=num, n_src=n_src, n_dst=n_dst)


def _oracle(kind, feats, w, g, geo):
    kw = dict(subm=True) if kind == "subm" else dict(inverse=True) if kind == "inverse" else {}
    ref = oracle.indice_conv(feats, w, geo["pairs"], geo["num"], geo["n_dst"], **kw)
    din, dw = oracle.indice_conv_backward(feats, w, g, geo["pairs"], geo["num"], **kw)
    return ref.numpy(), din.numpy(), dw.numpy()


@functools.lru_cache(maxsize=None)
def exact_case(kind, cin, cout, rows=ROWS, batch=BATCH, shape=tuple(SHAPE)):
    seed = _seed(kind, cin, cout, rows)
    geo = geometry(kind, batch, tuple(shape), rows, seed)
    rng = np.random.default_rng(seed + 1)
    tern = lambda size: (rng.integers(-1, 2, size=size) * (rng.random(size) < 0.375)).astype(np.float32)   # 2/3 * 3/8 = 1/4 non-zero
    feats, g = tern((geo["n_src"], cin)), tern((geo["n_dst"], cout))
    w = rng.integers(-1, 2, size=(3, 3, 3, cin, cout)).astype(np.float32)
    bias = rng.integers(-2, 3, size=(cout,)).astype(np.float32) if kind == "strided" else None
    ref, din, dw = _oracle(kind, feats, w, g, geo)
    if bias is not None:
        ref = ref + bias
    case = dict(geo, kind=kind, cin=cin, cout=cout, batch=batch, shape=list(shape), feats=feats, w=w, bias=bias, g=g, ref=ref, din=din, dw=dw)
    for name in ("ref", "din", "dw"):
        assert np.abs(case[name]).max() <= EXACT_MAX, (kind, cin, cout, rows, name, float(np.abs(case[name]).max()))
        assert np.array_equal(case[name], np.round(case[name]))
    return case


def exact_case_ids():
    """Arguments of every exact case the GPU test runs (the CPU test checks the <= 256 condition on all of them)."""
    ids = [(kind, cin, cout, ROWS, BATCH, tuple(SHAPE)) for kind in KINDS for cin, cout in CHANNELS]
    ids += [("subm", cin, cout, rows, EDGE_BATCH, tuple(EDGE_SHAPE)) for cin, cout in EDGE_CHANNELS for rows in EDGE_ROWS]
    return ids


def round_to(a, dtype):
    """float64 array of `a` rounded (to nearest even) to the torch dtype."""
    return torch.from_numpy(np.asarray(a, np.float32)).to(dtype).double().numpy()


@functools.lru_cache(maxsize=None)
def random_case(kind, cin, cout, dtype, rows=ROWS, batch=BATCH, shape=tuple(SHAPE)):
    """Operands are float64 arrays holding values of `dtype`.  ref / din / dw: float64 results; s_ref / s_din / s_dw: the sums of the
    absolute values of their terms; n_ref / n_din: terms per element of the row convs (kvol * gathered channels), n_dw [K]: pairs per
    offset."""
    assert kind in ("subm", "strided")
    seed = _seed(kind, cin, cout, rows) + 50000
    geo = geometry(kind, batch, tuple(shape), rows, seed)
    rng = np.random.default_rng(seed + 1)
    draw = lambda size: round_to(rng.standard_normal(size), dtype)
    feats, g, w = draw((geo["n_src"], cin)), draw((geo["n_dst"], cout)), draw((3, 3, 3, cin, cout))
    ref, din, dw = _oracle(kind, feats, w, g, geo)
    s_ref, s_din, s_dw = _oracle(kind, np.abs(feats), np.abs(w), np.abs(g), geo)
    assert ref.dtype == np.float64 and dw.dtype == np.float64
    return dict(geo, kind=kind, cin=cin, cout=cout, batch=batch, shape=list(shape), feats=feats, w=w, bias=None, g=g, ref=ref, din=din, dw=dw,
                s_ref=s_ref, s_din=s_din, s_dw=s_dw, n_ref=27 * cin, n_din=27 * cout, n_dw=np.asarray(geo["num"], np.int64))
