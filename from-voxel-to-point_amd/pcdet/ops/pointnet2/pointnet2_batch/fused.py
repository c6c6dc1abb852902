"""Fused grid set-abstraction (csrc/sa_fused.hip): what PointnetSAModuleMSG.forward (pointnet2_modules.py:30-62)
does after its ball query, for the bn=False shared MLP of the RoI head, without the grouped (R, C, M, S) tensor:

    sa_grid_max(per_point, per_centre, idx, w2)[r, i, :] = max_s relu(w2 @ relu(per_point[r, idx[r, i, s]] - per_centre[r, i]))

per_point (R, N, 64) / per_centre (R, M, 64) are the first (linear) shared-MLP layer applied to the points and to the centres,
idx (R, M, S) the ball-query result, w2 (64, 64) the second layer's 1x1-conv weight.  Gradients for per_point, per_centre and
w2 (the forward pass keeps one byte per centre and channel: which sample attained the maximum).  GPU only; `supported()` tells whether the kernel covers a shape (64 channels, 16 or 32 samples, N <= 884; backward runs eight waves per workgroup up to N = 589).

float16 / bfloat16 rows take the 16-bit MFMA kernels (fv2p_sa_grid_fwd_h / fv2p_sa_grid_bwd_h: 16-bit storage, fp32 accumulation, one
rounding, any N): per_point, per_centre and the incoming gradient share that dtype, w2 has it too or is float32 (the Conv2d parameter
beside autocast rows; it is rounded inside the kernel).  The output and the row gradients come back in the rows' dtype, grad_w2 in
w2's.  The per-point gradient has the fixed-order form only: the deterministic switch changes nothing there."""
import torch

import fv2p_native as _nat

from ... import _glue as G


def supported(per_point, idx):
    if not (per_point.is_cuda and per_point.dim() == 3 and idx.dim() == 3):
        return False
    dims = (per_point.shape[1], idx.shape[1], idx.shape[2], per_point.shape[2])
    if per_point.dtype == torch.float32:
        return bool(_nat.lib().fv2p_sa_grid_supported(*dims))
    if per_point.dtype in G.DT16:
        return bool(_nat.lib().fv2p_sa_grid_supported_h(*dims))
    return False


def _weight_code(w2, dt):
    """The `wd` of the *_h entry points: 0 for a float32 weight, the rows' dtype code for a weight of the rows' dtype."""
    if w2.dtype == torch.float32:
        return 0
    if w2.dtype != dt:
        raise TypeError(f"sa_grid_max: w2 must have the rows' dtype {dt} or be float32, got {w2.dtype} (nothing is cast here)")
    return G.DT16[dt]


def _fwd(saved, per_point, per_centre, idx, w2):
    r, n, c = per_point.shape
    m, s = idx.shape[1], idx.shape[2]
    dt = G.one_dtype("sa_grid_max", "per_point and per_centre", per_point, per_centre)
    per_point, per_centre, w2 = per_point.contiguous(), per_centre.contiguous(), w2.contiguous()
    out = G.new(per_point, (r, m, c), dt)
    need = per_point.requires_grad or per_centre.requires_grad or w2.requires_grad
    arg = G.new(per_point, (r, m, c), torch.uint8) if need else None   # which sample attained each maximum: all that backward needs
    if dt in G.DT16:
        G.run("fv2p_sa_grid_fwd_h", per_point, per_centre, idx, w2, _weight_code(w2, dt), r, n, m, s, c, out, arg, G.DT16[dt])
    else:
        G.run("fv2p_sa_grid_fwd", per_point, per_centre, idx, w2, r, n, m, s, c, out, arg)
    saved.update(t=(per_point, per_centre, idx, w2, arg), dims=(r, n, m, s, c))
    return out


def _bwd(saved, grad):
    per_point, per_centre, idx, w2, arg = saved["t"]
    if arg is None:
        raise RuntimeError("sa_grid_max: backward of a forward pass that ran without gradients enabled")
    r, n, m, s, c = saved["dims"]
    dt = G.one_dtype("sa_grid_max", "per_point, per_centre and the incoming gradient", per_point, per_centre, grad)
    g_point, g_centre, g_w = torch.empty_like(per_point), torch.empty_like(per_centre), torch.empty_like(w2)
    if dt in G.DT16:   # fixed order, no atomics: the only form, whatever the deterministic switch says
        ws = G.scratch("fv2p_sa_grid_bwd_h_ws_bytes", grad.device, r, m, s)
        G.run("fv2p_sa_grid_bwd_h", per_point, per_centre, idx, w2, _weight_code(w2, dt), arg, grad.contiguous(), r, n, m, s, c, g_point, g_centre,
              g_w, G.DT16[dt], ws, ws.numel())
        return g_point, g_centre, None, g_w
    if _nat.deterministic():   # per-point gradient in the fixed order of fv2p_scatter_add instead of LDS atomics
        ws = G.scratch("fv2p_sa_grid_bwd_gather_ws_bytes", grad.device, r, m, s)
        G.run("fv2p_sa_grid_bwd_gather", per_point, per_centre, idx, w2, arg, grad.contiguous(), r, n, m, s, c, g_point, g_centre, g_w, ws,
              ws.numel())
        return g_point, g_centre, None, g_w
    ws = G.scratch("fv2p_sa_grid_bwd_ws_bytes", grad.device, r)
    G.run("fv2p_sa_grid_bwd", per_point, per_centre, idx, w2, arg, grad.contiguous(), r, n, m, s, c, g_point, g_centre, g_w, ws, ws.numel())
    return g_point, g_centre, None, g_w


SaGridMax = G.autograd_op("SaGridMax", _fwd, _bwd)
sa_grid_max = SaGridMax.apply
