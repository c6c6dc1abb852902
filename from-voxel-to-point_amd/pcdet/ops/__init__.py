import os as _os
import sys as _sys

# fv2p_native (ctypes binding of libfv2p_ops.so) sits next to the pcdet package.
_root = _os.path.dirname(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
if _root not in _sys.path:
    _sys.path.insert(0, _root)


def set_deterministic(on):
    """Deterministic mode, process-wide (like spconv.set_bn_fold): with it on, every backward pass of pcdet.ops that would add with
    float atomics takes its fixed-order form instead, so a training step gives the same bits twice ("Deterministic
    mode").  Off by default; independent of torch.use_deterministic_algorithms."""
    import fv2p_native
    fv2p_native.set_deterministic(on)


def is_deterministic():
    import fv2p_native
    return fv2p_native.deterministic()
