"""Host side of the stacked voxeliser (fv2p_points_to_voxel_stack / points_to_voxel_stack): the three symbols are declared and exported,
the workspace query is a pure host function that never shrinks when an argument grows, the Python wrapper refuses bad arguments before
it reaches the library, and the expectation the GPU tests compare against is itself held against direct per-cloud calls.  No GPU is
needed."""
import ctypes
import os

import numpy as np
import pytest
import torch

import fv2p_native as nat
import oracle
import voxel_stack_cases as vc
from fv2p_harness import synth

SYMBOLS = ("fv2p_points_to_voxel_stack_ws_bytes", "fv2p_points_to_voxel_stack", "fv2p_points_to_voxel_stack_mean")


def _lib():
    """The shared object through plain ctypes: no HIP call is made by loading it or by the workspace query."""
    if not os.path.exists(nat.LIB_PATH):
        pytest.fail(f"{nat.LIB_PATH} is missing: build() first")
    return nat.lib()


def test_symbols_are_declared_in_the_header_and_exported():
    protos = nat.declared_symbols()
    for name in SYMBOLS:
        assert name in protos, f"{name} is not declared in include/fv2p_ops.h"
        assert hasattr(_lib(), name), f"{name} is not exported by libfv2p_ops.so"
    q, f, m = (protos[s] for s in SYMBOLS)
    assert q.restype is ctypes.c_size_t and [k for k, _, _ in q.params] == ["scalar"] * 3
    head = ["ptr", "scalar", "scalar", "scalar", "ptr", "hostarr", "hostarr", "hostarr", "scalar", "scalar"]
    assert f.restype is ctypes.c_int and [k for k, _, _ in f.params] == head + ["ptr"] * 5 + ["scalar", "scalar"]
    assert m.restype is ctypes.c_int and [k for k, _, _ in m.params] == head + ["ptr"] * 4 + ["scalar", "scalar"]
    assert f.params[-2][1] is ctypes.c_size_t and m.params[-2][1] is ctypes.c_size_t


@pytest.mark.parametrize("n,b,mv", [(1, 1, 1), (777, 2, 100), (16384, 1, 16000), (57884, 4, 16000), (131072, 8, 16000), (330000, 2, 80000),
                                    (360000, 2, 150000), (5000, 300, 7)])
def test_workspace_query_is_positive_and_never_decreases(n, b, mv):
    ws = _lib().fv2p_points_to_voxel_stack_ws_bytes
    base = ws(n, b, mv)
    assert base > 0
    for step in (1, 2, 255, 256, 1023, 2048, 4096, 30000, 1 << 20):
        assert ws(n + step, b, mv) >= base, ("n_total", step)
        assert ws(n, b + step, mv) >= base, ("batch", step)
        assert ws(n, b, mv + step) >= base, ("max_voxels", step)
    prev = [base, base, base]
    for d in range(1, 600):   # one at a time, across the primitives' tile boundaries
        cur = [ws(n + d, b, mv), ws(n, b + d, mv), ws(n, b, mv + d)]
        assert all(c >= p for c, p in zip(cur, prev)), (n, b, mv, d)
        prev = cur


def test_workspace_query_covers_the_single_cloud_query():
    """One cloud needs no less room stacked than alone: the same table, words and sort space plus the per-sample arrays."""
    for n, mv in [(1, 1), (4096, 16000), (16384, 16000), (180000, 150000)]:
        assert _lib().fv2p_points_to_voxel_stack_ws_bytes(n, 1, mv) >= _lib().fv2p_points_to_voxel_ws_bytes(n, min(n, mv))


def _wrappers():
    from pcdet.datasets.processor import voxel_generator as vg
    return vg.points_to_voxel_stack, vg.points_to_voxel_stack_list


def _no_library(monkeypatch):
    """Any library call from here on fails the test: the checks under test come first."""
    def boom(*a, **k):
        raise AssertionError("the library was reached before the arguments were checked")
    monkeypatch.setattr(nat, "call", boom)
    monkeypatch.setattr(nat, "lib", boom)
    monkeypatch.setattr(nat, "workspace", boom)


class _Cuda(torch.Tensor):
    """A CPU tensor that claims to live on the GPU: lets the argument checks that follow the device check run without one."""
    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t)

    @property
    def is_cuda(self):
        return True


def test_wrappers_are_exported_beside_the_batch_route():
    from pcdet.datasets.processor import voxel_generator as vg
    assert all(callable(f) for f in (vg.points_to_voxel_stack, vg.points_to_voxel_stack_list, vg.points_to_voxel_batch, vg.points_to_voxel))


def test_wrapper_rejects_a_cpu_tensor(monkeypatch):
    _no_library(monkeypatch)
    stack, as_list = _wrappers()
    with pytest.raises(nat.Fv2pError):
        stack(torch.zeros(10, 4), [4, 6], synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, 100)
    with pytest.raises(nat.Fv2pError):
        as_list([torch.zeros(4, 4), torch.zeros(6, 4)], synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, 100, mean_vfe=True)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float16, torch.int32])
def test_wrapper_rejects_a_wrong_dtype(monkeypatch, dtype):
    _no_library(monkeypatch)
    with pytest.raises(TypeError):
        _wrappers()[0](_Cuda(torch.zeros(10, 4, dtype=dtype)), [4, 6], synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, 100)


@pytest.mark.parametrize("shape", [(10, 2), (10, 1), (10,), (2, 5, 4)])
def test_wrapper_rejects_fewer_than_three_columns_and_wrong_ranks(monkeypatch, shape):
    _no_library(monkeypatch)
    with pytest.raises(ValueError):
        _wrappers()[0](_Cuda(torch.zeros(shape)), [4, 6], synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, 100)


@pytest.mark.parametrize("counts", [[4, 5], [6, 6], [10, 1], [11, -1], [-3, 13], []])
def test_wrapper_rejects_bad_counts(monkeypatch, counts):
    """Counts that do not sum to the rows, negative counts, an empty batch - as a list and as int32 / int64 tensors."""
    _no_library(monkeypatch)
    pts = _Cuda(torch.zeros(10, 4))
    for cnt in (counts, torch.tensor(counts, dtype=torch.int32), torch.tensor(counts, dtype=torch.int64)):
        with pytest.raises(ValueError):
            _wrappers()[0](pts, cnt, synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, 100)
    with pytest.raises(ValueError):
        _wrappers()[0](pts, torch.tensor([4.0, 6.0]), synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, 100)


def test_list_wrapper_rejects_an_empty_list_and_mixed_widths(monkeypatch):
    _no_library(monkeypatch)
    as_list = _wrappers()[1]
    with pytest.raises(ValueError):
        as_list([], synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, 100)
    with pytest.raises(ValueError):
        as_list([_Cuda(torch.zeros(4, 4)), _Cuda(torch.zeros(6, 5))], synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, 100)


@pytest.mark.parametrize("seed", range(12))
def test_expectation_builder_equals_direct_per_cloud_calls(seed):
    """Checks the checker: vc.expect is the per-cloud oracle output, cloud by cloud, with the sample column in front; every cloud keeps
    at most max_voxels rows and the random cases hit the break in some samples and miss it in others over the seeds."""
    clouds, vs, rng, mp, mv = vc.random_geometry(seed)
    if seed % 3 == 0:
        clouds.insert(seed % (len(clouds) + 1), np.zeros((0, clouds[0].shape[1]), np.float32))   # an empty cloud somewhere
    v, c, k, cnt = vc.expect(clouds, vs, rng, mp, mv)
    assert v.dtype == np.float32 and c.dtype == np.int32 and k.dtype == np.int32 and cnt.dtype == np.int32
    assert v.shape == (cnt.sum(), mp, clouds[0].shape[1]) and c.shape == (cnt.sum(), 4) and k.shape == (cnt.sum(),)
    row = 0
    for b, pts in enumerate(clouds):
        if pts.shape[0] == 0:
            assert cnt[b] == 0
            continue
        ov, oc, ok = oracle.points_to_voxel(pts, vs, rng, mp, mv)
        m = oc.shape[0]
        assert cnt[b] == m <= mv
        assert np.array_equal(v[row:row + m], ov) and np.array_equal(k[row:row + m], ok)
        assert np.array_equal(c[row:row + m, 1:], oc) and np.all(c[row:row + m, 0] == b)
        row += m
    assert row == c.shape[0]
    # the host entry point of the library gives the same rows (a second, independent implementation of the reference loop)
    from pcdet.datasets.processor.voxel_generator import points_to_voxel_host
    b = max(range(len(clouds)), key=lambda i: clouds[i].shape[0])
    hv, hc, hk = points_to_voxel_host(clouds[b], vs, rng, mp, True, mv)
    sel = c[:, 0] == b
    assert np.array_equal(v[sel], hv) and np.array_equal(c[sel, 1:], hc) and np.array_equal(k[sel], hk)


def test_random_cases_hit_the_break_in_a_good_share_of_samples():
    """Over the twelve seeds between a quarter and three quarters of the samples are cut off at max_voxels, and at least four stacks
    hold both kinds of sample."""
    hit, total, mixed = 0, 0, 0
    for seed in range(12):
        clouds, vs, rng, mp, mv = vc.random_geometry(seed)
        cut = [oracle.points_to_voxel(p, vs, rng, mp, 1 << 20)[1].shape[0] > mv for p in clouds]
        hit, total, mixed = hit + sum(cut), total + len(cut), mixed + (0 < sum(cut) < len(cut))
    assert 0.25 <= hit / total <= 0.75 and mixed >= 4, (hit, total, mixed)


def test_mean_expression_equals_the_padded_batch_expression():
    """vc.mean_of (slot-by-slot float32 sums) is MeanVFE over the padded voxels: sum over the slots / clamp_min(num, 1).  torch may
    add the slots in another order: at most 8 terms of magnitude below 64 differ by less than 8 * 64 * 2^-23 = 6.1e-5 before the
    division by a count >= 1."""
    clouds, vs, rng, mp, mv = vc.random_geometry(3)
    v, c, k, _ = vc.expect(clouds, vs, rng, mp, mv)
    assert mp <= 8 and np.abs(v).max() < 64
    tv, tk = torch.from_numpy(v), torch.from_numpy(k)
    want = tv.sum(dim=1) / torch.clamp_min(tk.view(-1, 1), 1.0).type_as(tv)
    assert np.abs(vc.mean_of(v, k) - want.numpy()).max() <= 6.1e-5
