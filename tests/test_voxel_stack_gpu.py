"""GPU parity of the stacked voxeliser (fv2p_points_to_voxel_stack / points_to_voxel_stack): a batch of unequal clouds in one call
against the oracle run per cloud and collated on the host (tests/voxel_stack_cases.py).

Bar, as tests/test_voxel_gpu.py: every output is bit-exact - coords, per-voxel counts and the float payload."""
import numpy as np
import pytest
import torch

import fv2p_native as nat
import oracle
import voxel_stack_cases as vc
from fv2p_harness import synth
from pcdet.datasets.processor.voxel_generator import (_grid_size, points_to_voxel, points_to_voxel_batch, points_to_voxel_host,
                                                      points_to_voxel_stack, points_to_voxel_stack_list)

pytestmark = pytest.mark.gpu


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def check(gpu, clouds, vs, rng, mp, mv, oracle_clouds=None):
    """Both forms of one stacked call against the expectation; returns the padded form's numpy outputs.
    oracle_clouds: what the oracle is given instead of clouds (it has no answer for NaN coordinates)."""
    ndim = clouds[0].shape[1]
    stacked = T(np.concatenate(clouds), gpu)
    cnt = [c.shape[0] for c in clouds]
    v, c, k = points_to_voxel_stack(stacked, cnt, vs, rng, mp, mv)
    assert v.is_cuda and c.is_cuda and k.is_cuda
    assert v.dtype == torch.float32 and c.dtype == torch.int32 and k.dtype == torch.int32
    ev, ec, ek, _ = vc.expect(clouds if oracle_clouds is None else oracle_clouds, vs, rng, mp, mv, ndim)
    v, c, k = v.cpu().numpy(), c.cpu().numpy(), k.cpu().numpy()
    assert c.shape == ec.shape and np.array_equal(c, ec)
    assert np.array_equal(k, ek)
    assert v.shape == ev.shape and np.array_equal(v, ev)
    f, c2 = points_to_voxel_stack(stacked, cnt, vs, rng, mp, mv, mean_vfe=True)
    assert f.dtype == torch.float32 and c2.dtype == torch.int32
    assert np.array_equal(c2.cpu().numpy(), ec)
    assert f.shape == (ec.shape[0], ndim) and np.array_equal(f.cpu().numpy(), vc.mean_of(ev, ek))
    return v, c, k


KITTI_SIZES = (14000, 16384, 9000, 18500)


@pytest.mark.parametrize("mv", [16000, 4000])
def test_stack_matches_oracle_on_seeded_kitti_clouds(gpu, mv):
    """Unequal KITTI crops; at max_voxels = 4000 some samples hit the break and others do not in the same call."""
    clouds = [synth.lidar_cloud(40 + b, n) for b, n in enumerate(KITTI_SIZES)] + [synth.lidar_cloud(50, 2500)]
    distinct = [oracle.points_to_voxel(p, synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, 1 << 20)[1].shape[0] for p in clouds]
    if mv == 4000:
        assert any(d > mv for d in distinct) and any(d <= mv for d in distinct), distinct
    else:
        assert all(d <= mv for d in distinct), distinct
    check(gpu, clouds, synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, mv)


@pytest.mark.parametrize("seed", range(14))
def test_stack_random_geometries_match_oracle(gpu, seed):
    clouds, vs, rng, mp, mv = vc.random_geometry(seed)
    check(gpu, clouds, vs, rng, mp, mv)


def test_stack_waymo_shape(gpu):
    clouds = [synth.waymo_like_cloud(5, 180000), synth.waymo_like_cloud(6, 150000)]
    check(gpu, clouds, synth.WAYMO_VOXEL, synth.WAYMO_RANGE, 5, 80000)


@pytest.mark.parametrize("where", ["first", "middle", "last", "all_but_one"])
def test_stack_with_empty_clouds(gpu, where):
    full = [synth.lidar_cloud(60 + b, n) for b, n in enumerate((3000, 777, 5000))]
    empty = np.zeros((0, 4), np.float32)
    clouds = {"first": [empty] + full, "middle": full[:1] + [empty, empty] + full[1:], "last": full + [empty],
              "all_but_one": [empty, empty, full[1], empty]}[where]
    v, c, k = check(gpu, clouds, synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, 2000)
    assert set(np.unique(c[:, 0])) == {b for b, p in enumerate(clouds) if p.shape[0]}


def test_stack_of_empty_clouds_only(gpu):
    pts = torch.zeros((0, 4), dtype=torch.float32, device=gpu)
    v, c, k = points_to_voxel_stack(pts, [0, 0, 0], synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, 100)
    assert v.shape == (0, 5, 4) and c.shape == (0, 4) and k.shape == (0,)
    f, c = points_to_voxel_stack(pts, [0], synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, 100, mean_vfe=True)
    assert f.shape == (0, 4) and c.shape == (0, 4)


def test_stack_edge_cases(gpu):
    near = synth.lidar_cloud(70, 1200)
    # a cloud entirely out of range between two ordinary ones
    out = np.full((100, 4), 1000.0, np.float32)
    v, c, k = check(gpu, [near, out, near[:500]], synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, 100000)
    assert not np.any(c[:, 0] == 1)
    # every point of a sample in ONE voxel, more than max_points
    one = np.tile(np.array([[10.01, 0.01, -1.01, 0.5]], np.float32), (1000, 1))
    one[:, 3] = np.arange(1000)
    v, c, k = check(gpu, [near, one, near[:500]], synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, 100000)
    sel = c[:, 0] == 1
    assert sel.sum() == 1 and int(k[sel][0]) == 5 and np.array_equal(v[sel][0, :, 3], np.arange(5, dtype=np.float32))
    # max_voxels = 1: the break on a sample's second voxel loses the later points of its first voxel too; its neighbours, one voxel
    # each, are untouched
    brk = np.array([[10.01, 0.01, -1.01, 0], [20.0, 0.0, -1.0, 1], [10.02, 0.01, -1.01, 2]], np.float32)
    left = np.array([[30.01, 1.01, -1.01, 7], [30.02, 1.01, -1.01, 8], [30.03, 1.01, -1.01, 9]], np.float32)
    right = np.array([[10.01, 0.01, -1.01, 4], [10.02, 0.01, -1.01, 5]], np.float32)
    v, c, k = check(gpu, [left, brk, right], synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, 1)
    assert k.tolist() == [3, 1, 2] and c[:, 0].tolist() == [0, 1, 2]
    # NaN coordinates are dropped: the sample comes out as if those points were not there (the oracle, like the reference loop, indexes
    # its dense map with them, so it is given the cloud without them), and as the library's host entry point voxelises it with them
    nan = near.copy()
    nan[::7, 0] = np.nan
    nan[3::11, 2] = np.nan
    clean = nan[~np.isnan(nan[:, :3]).any(axis=1)]
    assert 0 < clean.shape[0] < nan.shape[0]
    v, c, k = check(gpu, [near[:300], nan, near[:100]], synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, 500, [near[:300], clean, near[:100]])
    hv, hc, hk = points_to_voxel_host(nan, synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, True, 500)
    sel = c[:, 0] == 1
    assert np.array_equal(v[sel], hv) and np.array_equal(c[sel, 1:], hc) and np.array_equal(k[sel], hk)


@pytest.mark.parametrize("n,mv", [(16384, 16000), (16384, 3000), (50000, 40000), (1, 5)])
def test_stack_of_one_cloud_equals_points_to_voxel(gpu, n, mv):
    pts = T(synth.lidar_cloud(80, n), gpu)
    v, c, k = points_to_voxel_stack(pts, [n], synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, mv)
    sv, sc, sk = points_to_voxel(pts, synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, True, mv)
    assert torch.equal(v, sv) and torch.equal(k, sk) and torch.equal(c[:, 1:], sc) and bool((c[:, 0] == 0).all())


def test_same_cloud_twice_gives_the_same_rows_twice(gpu):
    pts = synth.lidar_cloud(81, 12000)
    for mv in (16000, 2500):
        v, c, k = check(gpu, [pts, synth.lidar_cloud(82, 5000), pts], synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, mv)
        a, b = c[:, 0] == 0, c[:, 0] == 2
        assert a.sum() == b.sum() > 0
        assert np.array_equal(v[a], v[b]) and np.array_equal(k[a], k[b]) and np.array_equal(c[a, 1:], c[b, 1:])


def _c_entry(gpu, clouds, mp, mv, extra, mean):
    """The C entry point with output buffers of rows_cap + extra rows pre-filled with a sentinel -> (outputs, voxel_cnt, rows_cap)."""
    ndim = clouds[0].shape[1]
    pts = T(np.concatenate(clouds), gpu)
    cnt = torch.tensor([c.shape[0] for c in clouds], dtype=torch.int32)
    rows_cap = int(torch.clamp(cnt, max=mv).sum())
    vs, rng = np.asarray(synth.KITTI_VOXEL, np.float32), np.asarray(synth.KITTI_RANGE, np.float32)
    grid = [int(g) for g in _grid_size(vs, rng)]
    coords = torch.full((rows_cap + extra, 4), -77, dtype=torch.int32, device=gpu)
    vcnt = torch.full((len(clouds) + 3,), -77, dtype=torch.int32, device=gpu)
    ws = torch.empty(nat.lib().fv2p_points_to_voxel_stack_ws_bytes(pts.shape[0], len(clouds), mv), dtype=torch.uint8, device=gpu)
    if mean:
        feats = torch.full((rows_cap + extra, ndim), -77.0, dtype=torch.float32, device=gpu)
        nat.call("fv2p_points_to_voxel_stack_mean", pts, pts.shape[0], ndim, len(clouds), cnt, vs.tolist(), rng[:3].tolist(), grid, mp, mv,
                 feats, coords, vcnt, ws, ws.numel(), nat.stream())
        outs = (feats, coords)
    else:
        voxels = torch.full((rows_cap + extra, mp, ndim), -77.0, dtype=torch.float32, device=gpu)
        num = torch.full((rows_cap + extra,), -77, dtype=torch.int32, device=gpu)
        nat.call("fv2p_points_to_voxel_stack", pts, pts.shape[0], ndim, len(clouds), cnt, vs.tolist(), rng[:3].tolist(), grid, mp, mv,
                 voxels, coords, num, vcnt, ws, ws.numel(), nat.stream())
        outs = (voxels, coords, num)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs], vcnt.cpu().numpy(), rows_cap


@pytest.mark.parametrize("mean", [False, True])
@pytest.mark.parametrize("mv", [16000, 1500])
def test_rows_past_the_total_are_zero_and_counts_are_per_cloud(gpu, mv, mean):
    """The caller allocates rows_cap = sum of min(n_b, max_voxels) rows; the call writes all of them - the produced rows, then zeros -
    and nothing behind them; voxel_cnt holds the per-cloud voxel counts."""
    clouds = [synth.lidar_cloud(90, 6000), np.zeros((0, 4), np.float32), synth.lidar_cloud(91, 900), synth.lidar_cloud(92, 9000)]
    ev, ec, ek, ecnt = vc.expect(clouds, synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, mv)
    outs, vcnt, rows_cap = _c_entry(gpu, clouds, 5, mv, 64, mean)
    m = int(ecnt.sum())
    assert m < rows_cap, "the case must leave rows between the produced total and the allocation"
    assert np.array_equal(vcnt[:len(clouds)], ecnt) and np.all(vcnt[len(clouds):] == -77)
    want = (vc.mean_of(ev, ek), ec) if mean else (ev, ec, ek)
    for o, w in zip(outs, want):
        assert np.array_equal(o[:m], w)
        assert not np.any(o[m:rows_cap]), "rows at or beyond the produced total must be zero"
        assert np.all(o[rows_cap:] == -77), "the call wrote behind the rows the caller allocated for it"


@pytest.mark.parametrize("mv", [16000, 1000])
def test_stack_equals_the_existing_batch_route(gpu, mv):
    """(voxels, coords, num_points) and the mean form's (features, coords) are torch.equal to points_to_voxel_batch on the same clouds,
    also under max_voxels overflow; the list convenience and every way of passing the counts give the same tensors."""
    clouds = [T(synth.lidar_cloud(7 + b, 6000 + 500 * b), gpu) for b in range(3)]
    cnt = [p.shape[0] for p in clouds]
    stacked = torch.cat(clouds)
    v, c, k = points_to_voxel_stack(stacked, cnt, synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, mv)
    bv, bc, bk = points_to_voxel_batch(clouds, synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, mv)
    assert torch.equal(v, bv) and torch.equal(c, bc) and torch.equal(k, bk)
    f, fc = points_to_voxel_stack(stacked, cnt, synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, mv, mean_vfe=True)
    bf, bfc = points_to_voxel_batch(clouds, synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, mv, mean_vfe=True)
    assert torch.equal(fc, c) and torch.equal(fc, bfc) and torch.equal(f, bf)
    if mv == 1000:
        assert v.shape[0] == 3000
    lv, lc, lk = points_to_voxel_stack_list(clouds, synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, mv)
    assert torch.equal(lv, v) and torch.equal(lc, c) and torch.equal(lk, k)
    lf, lfc = points_to_voxel_stack_list(clouds, synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, mv, mean_vfe=True)
    assert torch.equal(lf, f) and torch.equal(lfc, c)
    for counts in (torch.tensor(cnt, dtype=torch.int32), torch.tensor(cnt), torch.tensor(cnt, dtype=torch.int32, device=gpu)):
        tv, tc, tk = points_to_voxel_stack(stacked, counts, synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, mv)
        assert torch.equal(tv, v) and torch.equal(tc, c) and torch.equal(tk, k)


def test_two_calls_give_identical_bits(gpu):
    """The result does not depend on the order in which the hash inserts land."""
    clouds = [synth.lidar_cloud(30 + b, n) for b, n in enumerate(KITTI_SIZES)]
    stacked, cnt = T(np.concatenate(clouds), gpu), list(KITTI_SIZES)
    for mv in (16000, 4000):
        first = points_to_voxel_stack(stacked, cnt, synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, mv)
        again = points_to_voxel_stack(stacked, cnt, synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, mv)
        assert all(torch.equal(a, b) for a, b in zip(first, again))
        f1 = points_to_voxel_stack(stacked, cnt, synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, mv, mean_vfe=True)
        f2 = points_to_voxel_stack(stacked, cnt, synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, mv, mean_vfe=True)
        assert all(torch.equal(a, b) for a, b in zip(f1, f2))
        assert torch.equal(f1[1], first[1])


def test_more_clouds_than_one_offset_launch_carries(gpu):
    """300 small clouds: the offsets reach the device in two launches of 256."""
    rng = np.random.default_rng(5)
    base = synth.lidar_cloud(95, 6000)
    cuts = np.sort(rng.integers(0, 6000, 299))
    clouds = np.split(base, cuts)
    assert len(clouds) == 300
    check(gpu, clouds, synth.KITTI_VOXEL, synth.KITTI_RANGE, 3, 12)


def test_library_refuses_what_it_cannot_pack(gpu):
    pts = torch.zeros((10, 4), dtype=torch.float32, device=gpu)
    with pytest.raises(nat.Fv2pError):   # grid volume 5.6e11 fits 2^40 once, not ten times
        points_to_voxel_stack(pts, [1] * 10, [0.002, 0.002, 0.01], synth.KITTI_RANGE, 5, 100)
    with pytest.raises(nat.Fv2pError):   # batch * max_voxels above 2^24
        points_to_voxel_stack(pts, [1] * 10, synth.KITTI_VOXEL, synth.KITTI_RANGE, 5, 2000000)
