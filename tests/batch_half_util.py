"""Shared by the tests of the 16-bit batch gather / grouping / interpolation entry points (test_batch_half_cpu.py,
test_batch_half_gpu.py, test_batch_half_chain_gpu.py)."""
import ctypes

import fv2p_native as nat
from exit_half_util import DT_CODE, DTYPES, PREC, bits, dtype_id, f64, round_to  # noqa: F401  (re-exported to the test modules)

NEW_SYMBOLS = ["fv2p_gather_points_h", "fv2p_gather_points_grad_h_ws_bytes", "fv2p_gather_points_grad_h",
               "fv2p_group_points_batch_h", "fv2p_group_points_batch_grad_h_ws_bytes", "fv2p_group_points_batch_grad_h",
               "fv2p_three_interpolate_batch_h", "fv2p_three_interpolate_batch_grad_h_ws_bytes", "fv2p_three_interpolate_batch_grad_h"]


def missing_symbols():
    """The new entry points the built library lacks.  The GPU modules fail on a non-empty answer before they launch anything: on a
    library without the 16-bit forms the Python layer would hand 16-bit memory to float kernels."""
    raw = ctypes.CDLL(nat.LIB_PATH)
    declared = nat.declared_symbols()
    return [s for s in NEW_SYMBOLS if s not in declared or not hasattr(raw, s)]
