"""GPU: csrc/iou3d.hip at its edges, bit for bit against the oracle (oracle/iou3d_oracle.c) on the constructed inputs of
tests/iou3d_cases.py.  The kernels hold three things the oracle does not: the early-out at the head of box_overlap, the bounding-circle
pre-test of the NMS tiles and the chunked, early-stopping greedy pass of fv2p_nms_batch.  Pairwise overlap / IoU / 3-D IoU on box families
at coincident edges, at gaps around the reference's 1e-2 corner margin, at extreme aspect ratios, far centres, large headings, zero extents
and footprints below the margin, and on pairs on either side of each shortcut's gate; NMS survivors on structures known in closed form at
every tile size, on the below-margin sets and on the gate pairs; the batched NMS on five unlike samples in one call, at every max_keep
that changes its chunk schedule.  tests/test_iou3d_cases_cpu.py checks every construction used here without a GPU.

Before circles_apart allowed for the corner margin (reach + 1.5e-2) three tests failed here, on the MI355X (scale, threshold: survivors of
the kernel / of the reference):  test_nms_on_footprints_below_the_corner_margin  0.003, 0.1: 78 / 20 (rows 0 1 2 3 4 5 6 7 8 9 10 12 ...
against 0 2 3 4 5 8 9 10 14 15 21 28 ...);  0.003, 0.5: 78 / 21;  0.01, 0.1: 31 / 27 (0 .. 10 13 ... against 0 .. 6 8 9 10 16 17 ...);
0.01, 0.5: 57 / 55;  scale 0.03 passed.  test_nms_of_the_gate_pairs: the 0.02-sized side-by-side pairs 1e-4 beyond the old reach kept
[0, 1] where the reference keeps [0].  test_batched_nms_of_unlike_samples: the tiny0.01 sample, 54 / 47 survivors at n = 1345, 27 / 25 at
64, 28 / 26 at 65, 32 / 29 at 129.  Every pairwise test and every structure passed before and after."""
import functools

import numpy as np
import pytest
import torch

import fv2p_native as _nat
import iou3d_cases as ic
import oracle
from pcdet.ops.iou3d_nms import iou3d_nms_cuda, iou3d_nms_utils

pytestmark = pytest.mark.gpu

FAMS = ic.families()
MIXED = np.concatenate(list(FAMS.values()))[np.random.default_rng(3).permutation(sum(b.shape[0] for b in FAMS.values()))]
GATE_PAIRS, GATE_META = ic.gate_pairs()


def pair_sets():
    """name -> (a, b): every family against itself and against car boxes (either way round), the gate pairs (every first box against
    every second one: the constructed pairs are the diagonal), and slices of all families mixed at the shapes where the launch has a tail."""
    sets = {}
    for name, b in FAMS.items():
        cars = ic.partner_cars(name)
        sets[name] = (b, b)
        sets[name + "_x_cars"] = (b, cars)
        sets["cars_x_" + name] = (cars, b)
    sets["gates"] = (GATE_PAIRS[:, 0].copy(), GATE_PAIRS[:, 1].copy())
    assert MIXED.shape[0] >= 258
    sets["1x1"] = (MIXED[:1], MIXED[1:2])
    sets["1xn"] = (MIXED[2:3], MIXED[3:100])
    sets["nx1"] = (MIXED[3:100], MIXED[2:3])
    sets["15x17"] = (MIXED[:15], MIXED[15:32])          # 255 pairs
    sets["16x16"] = (MIXED[:16], MIXED[16:32])          # 256: one block exactly
    sets["1x257"] = (MIXED[:1], MIXED[1:258])           # 257: one pair in the second block
    sets["257x1"] = (MIXED[1:258], MIXED[:1])
    return sets


PAIR_SETS = pair_sets()


@functools.lru_cache(maxsize=None)
def pair_reference(name):
    a, b = PAIR_SETS[name]
    return oracle.boxes_bev(a, b, "overlap"), oracle.boxes_bev(a, b, "iou"), oracle.boxes_iou3d(a, b)


@pytest.mark.parametrize("name", list(PAIR_SETS))
def test_pairwise_entry_points_equal_the_oracle(gpu, name):
    a, b = PAIR_SETS[name]
    want_ov, want_iou, want_3d = pair_reference(name)
    ta, tb = torch.from_numpy(np.ascontiguousarray(a)).to(gpu), torch.from_numpy(np.ascontiguousarray(b)).to(gpu)
    ov = torch.full((a.shape[0], b.shape[0]), -7.0, device=gpu)
    assert iou3d_nms_cuda.boxes_overlap_bev_gpu(ta, tb, ov) == 1
    ov = ov.cpu().numpy()
    differ = np.argwhere(ov != want_ov)
    assert differ.size == 0, (name, "overlap", differ[:4], [(ov[i, j], want_ov[i, j]) for i, j in differ[:4]])
    iou = iou3d_nms_utils.boxes_iou_bev(ta, tb).cpu().numpy()
    differ = np.argwhere(iou != want_iou)
    assert differ.size == 0, (name, "iou", differ[:4], [(iou[i, j], want_iou[i, j]) for i, j in differ[:4]])
    i3 = iou3d_nms_utils.boxes_iou3d_gpu(ta, tb).cpu().numpy()
    assert i3.shape == want_3d.shape and np.abs(i3 - want_3d).max() < 1e-6
    if name == "gates":          # what the early-out skips: exactly 0 on both sides, and the constructed pairs are on the diagonal
        d2 = ic.centre_distance(GATE_PAIRS) ** 2
        outside = d2 > ic.early_out_d2(GATE_PAIRS[:, 0], GATE_PAIRS[:, 1])
        assert outside.sum() == 8 and (np.diag(ov)[outside] == 0).all() and (np.diag(ov) > 0).sum() >= 10


def test_host_entry_equals_the_oracle_on_every_family():
    """boxes_bev_iou_cpu runs the same box_overlap (early-out included) on the host."""
    for name in list(FAMS) + ["gates", "1x257"]:
        a, b = PAIR_SETS[name]
        got = iou3d_nms_utils.boxes_bev_iou_cpu(np.ascontiguousarray(a), np.ascontiguousarray(b))
        assert np.array_equal(got, pair_reference(name)[1]), name


def test_batched_iou3d_with_eight_value_rows_and_padding(gpu):
    """fv2p_boxes_iou3d_batch: one sample per family, rows padded with zeros to 40, ground-truth rows of 8 values (class id last)."""
    names = list(FAMS)
    a = np.zeros((len(names), 40, 7), np.float32)
    for second in ("self", "cars"):
        nb = 40 if second == "self" else 16
        b = np.zeros((len(names), nb, 8), np.float32)
        for s, name in enumerate(names):
            fam = FAMS[name]
            other = fam if second == "self" else ic.partner_cars(name)
            a[s, :fam.shape[0]] = fam
            b[s, :other.shape[0], :7], b[s, :other.shape[0], 7] = other, 1 + s
        ta, tb = torch.from_numpy(a).to(gpu), torch.from_numpy(b).to(gpu)
        out = torch.full((len(names), 40, nb), -7.0, device=gpu)
        _nat.call("fv2p_boxes_iou3d_batch", ta, len(names), 40, tb, nb, 8, out, _nat.stream())
        for s, name in enumerate(names):
            want = oracle.boxes_iou3d(a[s], b[s, :, :7])
            assert np.abs(out[s].cpu().numpy() - want).max() < 1e-6, (name, second)
            assert torch.equal(out[s], iou3d_nms_utils.boxes_iou3d_gpu(ta[s], tb[s, :, :7].contiguous())), (name, second)
            n_a, n_b = FAMS[name].shape[0], (FAMS[name].shape[0] if second == "self" else 12)
            assert (out[s, n_a:] == 0).all() and (out[s, :, n_b:] == 0).all()           # padding rows: IoU 0
        assert float(out.max()) > 0.5


# ------------------------------------------------------------------------------------------------ NMS
def descending(n):
    return -np.arange(n, dtype=np.float32)


def device_nms(gpu, boxes, thresh, normal=False):
    """Survivors by nms_device (boxes in score order) and by iou3d_nms_utils.nms_gpu / nms_normal_gpu (scores given): both lists."""
    tb = torch.from_numpy(np.ascontiguousarray(boxes)).to(gpu)
    keep, cnt = iou3d_nms_cuda.nms_device(tb, float(thresh), normal)
    assert keep.dtype == torch.int64 and cnt.dtype == torch.int32 and cnt.shape == (1,)
    first = keep[:int(cnt.item())].cpu().numpy()
    fn = iou3d_nms_utils.nms_normal_gpu if normal else iou3d_nms_utils.nms_gpu
    second = fn(tb, torch.from_numpy(descending(boxes.shape[0])).to(gpu), float(thresh))[0].cpu().numpy()
    return first, second


@pytest.mark.parametrize("n", ic.NMS_SIZES)
def test_nms_structures_at_the_tile_boundaries(gpu, n):
    for name, (boxes, thresh, want, flat) in ic.structures(n).items():
        for normal in ((False, True) if flat else (False,)):
            ref = oracle.nms(boxes, descending(n), thresh, normal=normal)
            assert np.array_equal(ref, want), (name, n, normal)
            for got in device_nms(gpu, boxes, thresh, normal):
                assert len(got) == len(ref) and np.array_equal(got, ref), (name, n, normal, got, ref)


@pytest.mark.parametrize("thresh", [0.1, 0.5])
@pytest.mark.parametrize("scale", ic.TINY_SCALES)
def test_nms_on_footprints_below_the_corner_margin(gpu, scale, thresh):
    """200 boxes of scale * U(0.5, 2): at 0.003 and 0.01 most suppressions are between disjoint boxes less than the corner margin apart."""
    boxes = ic.tiny(scale, n=200)
    ref = oracle.nms(boxes, descending(200), thresh)
    for got in device_nms(gpu, boxes, thresh):
        print(f"tiny {scale:g} thresh {thresh}: reference keeps {len(ref)}, the kernel {len(got)}; kernel's first rows {got[:12].tolist()}, the reference's {ref[:12].tolist()}")
        assert len(got) == len(ref) and np.array_equal(got, ref)


def test_nms_of_the_gate_pairs(gpu):
    """Each gate pair as a two-box set at threshold 0: the second box falls exactly when the reference finds any overlap at all."""
    fell = 0
    for k, pair in enumerate(GATE_PAIRS):
        ref = oracle.nms(pair, descending(2), 0.0)
        for got in device_nms(gpu, pair, 0.0):
            assert np.array_equal(got, ref), (GATE_META[k], got, ref)
        fell += len(ref) == 1
    assert 10 <= fell < len(GATE_PAIRS)


# ------------------------------------------------------------------------------------------------ the batched, truncated NMS
@functools.lru_cache(maxsize=None)
def batch_reference(n):
    batch = ic.batch_case(n)
    return batch, [oracle.nms(batch[s], descending(n), ic.BATCH_THRESH) for s in range(batch.shape[0])]


def nms_batch_raw(gpu, boxes, max_keep, normal=False):
    """The C entry on a keep buffer of batch rows of keep_stride = K values (the layout is packed: row s starts at s * keep_stride) and one
    guard value behind the last row, all filled with -1 -> (keep [batch, K], the guard, counts)."""
    batch, n = boxes.shape[:2]
    stride = max(min(max_keep, n) if max_keep > 0 else n, 1)
    keep = torch.full((batch * stride + 1,), -1, dtype=torch.int64, device=gpu)
    cnt = torch.full((batch,), -1, dtype=torch.int32, device=gpu)
    ws = _nat.workspace(_nat.lib().fv2p_nms_batch_ws_bytes(batch, n, int(max_keep)), gpu)
    _nat.call("fv2p_nms_batch", boxes, batch, n, float(ic.BATCH_THRESH), int(normal), int(max_keep), keep, stride, cnt, ws, ws.numel(), _nat.stream())
    keep = keep.cpu().numpy()
    return keep[:-1].reshape(batch, stride), int(keep[-1]), cnt.cpu().numpy()


@pytest.mark.parametrize("n", ic.BATCH_SIZES)
def test_batched_nms_of_unlike_samples(gpu, n):
    """identical, disjoint, chain, a below-margin set and car boxes in one call: with max_keep = 1 or 2 the mask comes in chunks of
    1 + 4 + 16 + 1 row blocks at n = 1345, and the samples finish in different ones.  The head of every row is the head of the full
    survivor list, nothing is written behind a row, and a second call returns the same buffer."""
    batch, refs = batch_reference(n)
    tb = torch.from_numpy(batch).to(gpu)
    for max_keep in ic.max_keeps(n):
        keep, guard, cnt = nms_batch_raw(gpu, tb, max_keep)
        again = nms_batch_raw(gpu, tb, max_keep)
        assert guard == -1
        assert np.array_equal(keep, again[0]) and again[1] == -1 and np.array_equal(cnt, again[2])
        for s, ref in enumerate(refs):
            head = ref[:max_keep] if max_keep > 0 else ref
            assert cnt[s] == len(head), (ic.BATCH_SAMPLES[s], n, max_keep, cnt[s], len(head))
            assert np.array_equal(keep[s, :cnt[s]], head), (ic.BATCH_SAMPLES[s], n, max_keep)
            # a batch of one: the guard sits right behind this sample's row
            one, guard_one, cnt_one = nms_batch_raw(gpu, tb[s:s + 1].contiguous(), max_keep)
            assert guard_one == -1 and cnt_one[0] == len(head) and np.array_equal(one[0, :len(head)], head), (ic.BATCH_SAMPLES[s], n, max_keep)
        # the wrapper: same heads
        wk, wc = iou3d_nms_cuda.nms_batch_device(tb, float(ic.BATCH_THRESH), max_keep)
        assert wk.shape == (5, keep.shape[1]) and np.array_equal(wc.cpu().numpy(), cnt)
        for s in range(5):
            assert np.array_equal(wk[s, :cnt[s]].cpu().numpy(), keep[s, :cnt[s]])


@pytest.mark.parametrize("n", [65, 129])
def test_batched_normal_nms_of_the_axis_aligned_samples(gpu, n):
    """normal = 1 takes the other branch of nms_tile (no pre-test): identical (heading 0), disjoint, chain."""
    batch = np.stack([ic.identical(n)[0], ic.disjoint(n)[0], ic.chain(n)[0]])
    tb = torch.from_numpy(batch).to(gpu)
    refs = [oracle.nms(batch[s], descending(n), ic.BATCH_THRESH, normal=True) for s in range(3)]
    assert [len(r) for r in refs] == [1, n, (n + 1) // 2]
    for max_keep in ic.max_keeps(n):
        keep, guard, cnt = nms_batch_raw(gpu, tb, max_keep, normal=True)
        assert guard == -1
        for s, ref in enumerate(refs):
            head = ref[:max_keep] if max_keep > 0 else ref
            assert cnt[s] == len(head) and np.array_equal(keep[s, :cnt[s]], head), (s, n, max_keep)
