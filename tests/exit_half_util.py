"""Shared by the tests of the 16-bit dense() / group / grouping / interpolation entry points (test_exit_half_cpu.py,
test_dense_half_gpu.py, test_point_half_gpu.py, test_exit_half_chain_gpu.py)."""
import ctypes

import numpy as np
import torch

import fv2p_native as nat

NEW_SYMBOLS = ["fv2p_sparse_to_dense_h", "fv2p_dense_to_sparse_h", "fv2p_sparse_group_fwd_h", "fv2p_sparse_group_bwd_h",
               "fv2p_group_points_stack_h", "fv2p_group_points_stack_grad_h", "fv2p_group_points_stack_grad_h_ws_bytes",
               "fv2p_three_interpolate_stack_h", "fv2p_three_interpolate_stack_grad_h", "fv2p_three_interpolate_stack_grad_h_ws_bytes"]
DTYPES = [torch.float16, torch.bfloat16]
DT_CODE = {torch.float16: 1, torch.bfloat16: 2}
PREC = {torch.float16: 10, torch.bfloat16: 7}     # stored fraction bits p: one rounding is within 2^-(p+1) |value|
dtype_id = lambda d: str(d).replace("torch.", "")


def missing_symbols():
    """The new entry points the built library lacks.  The GPU modules fail on a non-empty answer before they launch anything: on a
    library without the 16-bit forms the Python layer would hand 16-bit memory to float kernels."""
    raw = ctypes.CDLL(nat.LIB_PATH)
    declared = nat.declared_symbols()
    return [s for s in NEW_SYMBOLS if s not in declared or not hasattr(raw, s)]


def bits(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy()


def f64(t):
    return t.detach().double().cpu().numpy()


def round_to(a, dtype):
    """float64 array rounded to nearest even ONCE into `dtype`, as a float64 array (torch rounds a double directly)."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dtype).double().numpy()
