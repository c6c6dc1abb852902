"""GPU: the bilinear gather of BEV features on float16 / bfloat16 maps (fv2p_bev_interp_fwd_h / _bwd_h, fv2p_transpose_batched_h) and
its Python front end `_BevInterp`.

  forward : bit-equal to fv2p_bev_interp_fwd on the widened map, rounded to the dtype (same corners, same fp32 expression, one rounding);
  backward: bit-equal to fv2p_bev_interp_bwd_gather on the widened gradient, rounded (both use the association of fv2p_scatter_add), and
            within u |ref64| + (k + 1) 2^-24 sum |w g| per cell of a float64 adjoint, k the cell's entry count: k fp32 products and k
            additions of the fixed-order sum, then ONE rounding to the format (u = 2^-11 / 2^-8);
  the 16-bit transpose equals .permute().contiguous() bit for bit; n = 0 launches nothing and still zero-fills the gradient; two runs are
  bit-identical; int8 and float64 maps still raise."""
import numpy as np
import pytest
import torch

import fv2p_native as nat
from pcdet.models.backbones_3d.pfe.bev_grid_pooling import _BevInterp

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]
DT_CODE = {torch.float16: 1, torch.bfloat16: 2}
UNIT = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
dtype_id = lambda d: str(d).replace("torch.", "")
BATCH = 2
FILL = 77.0


def points(h, w, seed):
    """x, y [BATCH, N] float32 (host): inside the map, on integer coordinates, on the last row / column, outside on every side, six points
    sharing one position, and 40 points on one cell (a row of more than 32 entries spans segments of the scatter).  Fractional parts are
    0 or lie in [1/8, 7/8]: a bilinear weight is 0 or at least 1/64 (see `cotangent`)."""
    rng = np.random.default_rng(seed)
    frac = lambda size: rng.uniform(0.125, 0.875, size=size)
    xs, ys = [], []
    for b in range(BATCH):
        x = list(rng.integers(0, w - 1, size=24) + frac(24)) + [0.0, 1.0, 2.0, w - 1.0, w - 1.0, 1.5, 0.25]
        y = list(rng.integers(0, h - 1, size=24) + frac(24)) + [0.0, 2.0, 1.0, h - 1.0, 1.25, h - 1.0, h - 1.0]
        x += [-1.5, w + 0.75, 1.25, 2.375, -0.25, w - 0.5]
        y += [1.25, 2.125, -2.25, h + 1.25, -0.625, h - 0.375]
        x += [2.75] * 6
        y += [1.5 + b] * 6
        x += list(1.0 + frac(40))
        y += list(3.0 + frac(40))
        xs.append(x)
        ys.append(y)
    return np.asarray(xs, np.float32), np.asarray(ys, np.float32)


def cotangent(n, c, dtype, seed):
    """[BATCH, n, c] host tensor of the dtype: magnitudes in [0.5, 2], one random sign per channel, so that only the negative weights of
    the points outside the map cancel anything.  With the weights of `points` a cell's total is then 0 or far above 2^-14 - below that a
    float16 result is subnormal and NO rounding to the format can meet u |ref|.  The test asserts that no cell of its data has such a
    total."""
    rng = np.random.default_rng(seed)
    g = rng.uniform(0.5, 2.0, size=(BATCH, n, c)) * rng.choice([-1.0, 1.0], size=(1, 1, c))
    return torch.from_numpy(g).to(dtype)


def corners_host(x, y, h, w):
    """bev_corners in numpy float32: cell indices [4][B, N] and weights [4][B, N] (float32 values, one rounding per operation)."""
    f = np.float32
    x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    x1, y1 = x0 + 1, y0 + 1
    x0, x1, y0, y1 = np.clip(x0, 0, w - 1), np.clip(x1, 0, w - 1), np.clip(y0, 0, h - 1), np.clip(y1, 0, h - 1)
    fx0, fx1, fy0, fy1 = x0.astype(f), x1.astype(f), y0.astype(f), y1.astype(f)
    cells = [y0 * w + x0, y1 * w + x0, y0 * w + x1, y1 * w + x1]
    wts = [(fx1 - x) * (fy1 - y), (fx1 - x) * (y - fy0), (x - fx0) * (fy1 - y), (x - fx0) * (y - fy0)]
    assert all(v.dtype == f for v in wts)
    return cells, wts


def adjoint64(g, x, y, h, w):
    """g [B, N, C] float64 -> (grad [B, H*W, C], sum |w g| [B, H*W, C], entry count [B, H*W]) in float64"""
    b, n, c = g.shape
    cells, wts = corners_host(x, y, h, w)
    grad, mag, cnt = np.zeros((b, h * w, c)), np.zeros((b, h * w, c)), np.zeros((b, h * w))
    bi = np.repeat(np.arange(b), n)
    for cell, wt in zip(cells, wts):
        np.add.at(grad, (bi, cell.reshape(-1)), wt.astype(np.float64).reshape(-1, 1) * g.reshape(b * n, c))
        np.add.at(mag, (bi, cell.reshape(-1)), np.abs(wt.astype(np.float64).reshape(-1, 1) * g.reshape(b * n, c)))
        np.add.at(cnt, (bi, cell.reshape(-1)), 1.0)
    return grad, mag, cnt


def _offset(t, offset):
    if not offset:
        return t
    buf = torch.empty(t.numel() + offset, dtype=t.dtype, device=t.device)
    v = buf[offset:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0
    return v


def fwd32(bev32, x, y, cf):
    b, n = x.shape
    bsz, c, h, w = bev32.shape if cf else (bev32.shape[0], bev32.shape[3], bev32.shape[1], bev32.shape[2])
    out = torch.empty((b, n, c), dtype=torch.float32, device=bev32.device)
    ws = nat.workspace(max(nat.call("fv2p_bev_interp_ws_bytes", bsz, c, h, w, int(cf)), 16), bev32.device)
    nat.call("fv2p_bev_interp_fwd", bev32, bsz, c, h, w, int(cf), x, y, n, out, ws, ws.numel(), nat.stream())
    return out


def bwd32_gather(g32, x, y, c, h, w, cf):
    b, n = x.shape
    grad = torch.empty((b, c, h, w) if cf else (b, h, w, c), dtype=torch.float32, device=g32.device)
    ws = nat.workspace(nat.call("fv2p_bev_interp_bwd_ws_bytes", b, c, h, w, int(cf), n), g32.device)
    nat.call("fv2p_bev_interp_bwd_gather", g32, b, c, h, w, int(cf), x, y, n, grad, ws, ws.numel(), nat.stream())
    return grad


def bwd16_raw(g, x, y, c, h, w, cf, offset=0):
    b, n = x.shape
    shape = (b, c, h, w) if cf else (b, h, w, c)
    buf = torch.full((b * c * h * w + offset,), FILL, dtype=g.dtype, device=g.device)
    grad = buf[offset:].view(shape)
    ws = nat.workspace(max(nat.call("fv2p_bev_interp_bwd_h_ws_bytes", b, c, h, w, int(cf), n), 16), g.device)
    nat.call("fv2p_bev_interp_bwd_h", g if n else None, b, c, h, w, int(cf), x, y, n, grad, DT_CODE[g.dtype], ws, ws.numel(), nat.stream())
    return grad


def bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("c", [1, 7, 8, 64, 520])
@pytest.mark.parametrize("hw", [(5, 6), (16, 16)], ids=["5x6", "16x16"])
@pytest.mark.parametrize("cf", [True, False], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_gather_and_gradient_equal_the_fp32_ops_on_widened_operands(gpu, dtype, cf, hw, c):
    h, w = hw
    torch.manual_seed(c * 100 + h)
    xh, yh = points(h, w, c + h)
    x, y = torch.from_numpy(xh).to(gpu), torch.from_numpy(yh).to(gpu)
    n = x.shape[1]
    offset = 1 if c == 8 else 0     # c % 8 == 0 with a map pointer that is not 16-byte aligned: the element path
    bev = _offset(torch.randn((BATCH, c, h, w) if cf else (BATCH, h, w, c), device=gpu).to(dtype), offset).detach().requires_grad_(True)
    out = _BevInterp.apply(bev, x, y, cf)
    assert out.dtype == dtype and out.shape == (BATCH, n, c)
    ref = fwd32(bev.detach().float(), x, y, cf).to(dtype)
    assert torch.equal(bits(out), bits(ref))
    g_host = cotangent(n, c, dtype, 7 * c + h)
    g = g_host.to(gpu)
    out.backward(g)
    assert bev.grad.dtype == dtype and bev.grad.shape == bev.shape
    ref_g = bwd32_gather(g.float(), x, y, c, h, w, cf)
    assert torch.equal(bev.grad, ref_g.to(dtype))
    # nothing depends on the deterministic switch, and a second run gives the same bits
    nat.set_deterministic(True)
    try:
        again = bwd16_raw(g, x, y, c, h, w, cf)
    finally:
        nat.set_deterministic(False)
    assert torch.equal(bits(again), bits(bev.grad))
    assert torch.equal(bits(_BevInterp.apply(bev.detach(), x, y, cf)), bits(out))
    if offset:   # a gradient that is not 16-byte aligned either
        assert torch.equal(bits(bwd16_raw(g, x, y, c, h, w, cf, offset=1)), bits(bev.grad))
    # the float64 adjoint
    got = bev.grad.detach().double()
    got = (got.reshape(BATCH, c, h * w).permute(0, 2, 1) if cf else got.reshape(BATCH, h * w, c)).cpu().numpy()
    ref64, mag, cnt = adjoint64(g_host.double().numpy(), xh, yh, h, w)
    assert cnt.max() > 32
    assert ((ref64 == 0) | (np.abs(ref64) >= 2.0 ** -13)).all(), "a cell total in float16's subnormal range: choose other data"
    bound = UNIT[dtype] * np.abs(ref64) + (cnt[..., None] + 1) * 2.0 ** -24 * mag
    ratio = np.abs(got - ref64) / np.maximum(bound, 1e-300)
    print("max |err| / bound = %.3f, largest cell has %d entries" % (np.where(bound > 0, ratio, 0).max(), cnt.max()))
    assert (np.abs(got - ref64) <= bound).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_transpose_equals_permute_contiguous(gpu, dtype):
    sizes = [1, 7, 8, 64, 65, 200]
    for rows in sizes:
        for cols in sizes:
            for offset in ((0, 1) if (rows, cols) in ((8, 64), (64, 200), (200, 8)) else (0,)):
                src = _offset(torch.randn(3, rows, cols, device=gpu).to(dtype), offset)
                buf = torch.full((3 * rows * cols + offset,), FILL, dtype=dtype, device=gpu)
                dst = buf[offset:].view(3, cols, rows)
                nat.call("fv2p_transpose_batched_h", src, 3, rows, cols, dst, nat.stream())
                assert torch.equal(bits(dst), bits(src.permute(0, 2, 1))), (rows, cols, offset)
    # bit patterns are moved: NaN payloads and negative zeros survive
    raw = torch.randint(-32768, 32767, (2, 65, 72), dtype=torch.int16, device=gpu)
    out = torch.empty((2, 72, 65), dtype=torch.int16, device=gpu)
    nat.call("fv2p_transpose_batched_h", raw, 2, 65, 72, out, nat.stream())
    assert torch.equal(out, raw.permute(0, 2, 1).contiguous())


@pytest.mark.parametrize("cf", [True, False], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_no_points_still_zero_fill_the_gradient(gpu, dtype, cf):
    c, h, w = 8, 5, 6
    x = torch.empty((BATCH, 0), device=gpu)
    bev = torch.randn((BATCH, c, h, w) if cf else (BATCH, h, w, c), device=gpu).to(dtype)
    out = _BevInterp.apply(bev, x, x, cf)
    assert out.shape == (BATCH, 0, c) and out.dtype == dtype
    grad = bwd16_raw(torch.empty((BATCH, 0, c), dtype=dtype, device=gpu), x, x, c, h, w, cf)
    assert bool((grad == 0).all())


def test_other_dtypes_still_raise(gpu):
    x = torch.rand(1, 4, device=gpu)
    bev = torch.randn(1, 8, 5, 6, device=gpu)
    for bad in (bev.to(torch.int8), bev.double()):
        with pytest.raises(nat.Fv2pError):
            _BevInterp.apply(bad, x, x, True)
    assert _BevInterp.apply(bev, x, x, True).dtype == torch.float32
