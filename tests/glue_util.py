"""Shared by the suites of the target and loss kernels of csrc/targets.hip (test_roi_glue_gpu.py, test_anchor_loss_gpu.py,
test_anchor_assign_gpu.py): the switch to the tensor formulations and the gradient yardstick."""
import numpy as np

from fv2p_harness import fv2p_model as fm


class tensor_ops:
    """KERNEL_GLUE off: the tensor formulations on whatever device the tensors live on."""

    def __enter__(self):
        self.was, fm.KERNEL_GLUE = fm.KERNEL_GLUE, False

    def __exit__(self, *a):
        fm.KERNEL_GLUE = self.was


def hold(name, got, want, base):
    """got against the yardstick `want`, where the fp32 tensor form `base` is E away from it."""
    e = np.abs(base - want).max()
    err = np.abs(got - want).max()
    bound = 2 * e + 1e-7 * np.abs(want).max()
    print(f"{name}: E {e:.3e}  kernel error {err:.3e}  bound {bound:.3e}  max|grad| {np.abs(want).max():.3e}")
    assert np.isfinite(got).all() and err <= bound, name
