"""The oracle's stacked ball query, voxel query and 3-NN against the plain numpy references of tests/stack_cases.py, on EVERY case of the
builder: sample layouts with zero-query and zero-point samples, workgroup-sized and tile-sized counts, nsample 1 ... 100, exact ties and
exact d2 == r2 on the dyadic lattice.  This is what proves the cases and the references right on a machine without a GPU; the GPU file
(tests/test_pointnet2_stack_gpu.py) holds the HIP ops to both.  It also enforces, per case of the generic family, that at most 1 % of the
queries have a float64-borderline candidate, and that the float64 brute force agrees with the float32 reference on all the others - so a
bad seed fails here and not on the GPU.  CPU only."""
import numpy as np
import pytest

import oracle
import stack_cases as sc


def _check_float64(ref32, ref64, amb):
    """The 1 % condition and the float64 comparison on every query that is not borderline."""
    assert amb.sum() <= 0.01 * amb.size, f"{int(amb.sum())} of {amb.size} queries are float64-borderline: pick another seed"
    assert np.array_equal(ref32[~amb], ref64[~amb])


@pytest.mark.parametrize("case", sc.BALL_CASES, ids=sc.case_id)
def test_oracle_ball_query_stack(case):
    layout, family, radius, nsample = case
    c = sc.cloud_case(layout, family, radius)
    got = oracle.ball_query_stack(radius, nsample, c["xyz"], c["xyz_cnt"], c["new_xyz"], c["new_cnt"])
    ref32, hits = sc.ref_ball_query(c, nsample, sc.d2_f32)
    ref64, hits64 = sc.ref_ball_query(c, nsample, sc.d2_f64)
    assert got.dtype == np.int32 and np.array_equal(got, ref32)
    if family == "lattice":
        assert np.array_equal(ref32, ref64) and np.array_equal(hits, hits64)      # exact arithmetic: no borderline pair at all
        for q in c["planted"]["one_hit_last"]:
            assert hits[q] == 1                                                   # d2 == r2 and one step outside are both rejected
        for q in c["planted"]["only_at_radius"] + c["planted"]["remote"]:
            assert hits[q] == 0 and got[q, 0] == -1 and not got[q, 1:].any()
    else:
        _check_float64(ref32, ref64, sc.ambiguous_ball(c))
    # the single hit of the planted query is the sample's LAST row (behind a tile boundary for the 1025 / 2049-point samples)
    blocks = sc.sample_blocks(c["xyz_cnt"])
    bs_of = np.repeat(np.arange(len(blocks)), c["new_cnt"])
    for q in c["planted"]["one_hit_last"]:
        n = blocks[bs_of[q]][1] - blocks[bs_of[q]][0]
        assert (got[q] == n - 1).all()


def test_ball_cases_cover_what_they_claim():
    """Over the whole set: every nsample and both radii; balls with more hits than 64 and than nsample = 100, with exactly one hit, with
    fewer hits than nsample (padding) and with none; planted d2 == r2 pairs on the lattice."""
    seen_ns, seen_r, over64, over100, padded = set(), set(), 0, 0, 0
    for layout, family, radius, nsample in sc.BALL_CASES:
        c = sc.cloud_case(layout, family, radius)
        _, hits = sc.ref_ball_query(c, nsample, sc.d2_f32)
        seen_ns.add(nsample)
        seen_r.add(radius)
        over64 += int((hits > 64).sum()) if nsample >= 64 else 0
        over100 += int((hits > 100).sum()) if nsample == 100 else 0
        padded += int(((hits > 0) & (hits < nsample)).sum())
        if family == "lattice" and c["planted"]["only_at_radius"]:
            q = c["planted"]["only_at_radius"][0]
            (p0, p1), = [b for b, (q0, q1) in zip(sc.sample_blocks(c["xyz_cnt"]), sc.sample_blocks(c["new_cnt"])) if q0 <= q < q1]
            assert (sc.d2_f64(c["new_xyz"][q:q + 1], c["xyz"][p0:p1]) == float(sc.r2_of(radius))).sum() >= 2
    assert seen_ns == set(sc.NSAMPLES) and seen_r == set(sc.RADII)
    assert over64 > 100 and over100 > 100 and padded > 100


@pytest.mark.parametrize("family", ["lattice", "generic"])
def test_the_lattice_is_exact_and_the_generic_family_is_not(family):
    """Every pair of a lattice case has the same squared distance in ordered float32 and in float64."""
    c = sc.cloud_case("today", family, 1.25)
    same = []
    for (p0, p1), (q0, q1) in zip(sc.sample_blocks(c["xyz_cnt"]), sc.sample_blocks(c["new_cnt"])):
        same.append((sc.d2_f32(c["new_xyz"][q0:q1], c["xyz"][p0:p1]).astype(np.float64) == sc.d2_f64(c["new_xyz"][q0:q1], c["xyz"][p0:p1])).all())
    assert all(same) == (family == "lattice")
    s = sc.voxel_scene(family, 1.25)
    assert (sc.d2_f32(s["new_xyz"], s["xyz"]).astype(np.float64) == sc.d2_f64(s["new_xyz"], s["xyz"])).all() == (family == "lattice")


@pytest.mark.parametrize("case", sc.NN_CASES, ids=sc.case_id)
def test_oracle_three_nn_stack(case):
    layout, family = case
    c = sc.cloud_case(layout, family)
    d2, idx = oracle.three_nn_stack(c["new_xyz"], c["new_cnt"], c["xyz"], c["xyz_cnt"])
    rd32, ri32 = sc.ref_three_nn(c, sc.d2_f32)
    rd64, ri64 = sc.ref_three_nn(c, sc.d2_f64)
    assert np.array_equal(idx, ri32) and np.array_equal(d2, rd32)
    if family == "lattice":
        assert np.array_equal(ri32, ri64) and np.array_equal(rd32, rd64)
        for q in c["planted"]["tie3"]:
            assert d2[q, 0] == d2[q, 1] == d2[q, 2] and idx[q, 0] < idx[q, 1] < idx[q, 2]     # equal distances: row order
    else:
        _check_float64(ri32, ri64, sc.ambiguous_three_nn(c))
    # fewer than three known points: (+inf, first row of the sample) in the untouched slots
    for (p0, p1), (q0, q1) in zip(sc.sample_blocks(c["xyz_cnt"]), sc.sample_blocks(c["new_cnt"])):
        k = p1 - p0
        if k < 3 and q1 > q0:
            assert np.isinf(d2[q0:q1, k:]).all() and (idx[q0:q1, k:] == p0).all() and np.isfinite(d2[q0:q1, :k]).all()


def test_three_nn_lattice_cases_hold_four_way_ties():
    c = sc.cloud_case("today", "lattice")
    n = 0
    for q in c["planted"]["tie3"]:
        (p0, p1), = [b for b, (q0, q1) in zip(sc.sample_blocks(c["xyz_cnt"]), sc.sample_blocks(c["new_cnt"])) if q0 <= q < q1]
        s = np.sort(sc.d2_f64(c["new_xyz"][q:q + 1], c["xyz"][p0:p1])[0])
        n += int(s[2] == s[3])
    assert n >= 1      # a fourth point at exactly the third distance, with a higher row: it must stay out


@pytest.mark.parametrize("case", sc.VOXEL_CASES, ids=sc.case_id)
def test_oracle_voxel_query_stack(case):
    family, max_range, radius, nsample = case
    s = sc.voxel_scene(family, radius)
    got = oracle.voxel_query_stack(list(max_range), radius, nsample, s["xyz"], s["new_xyz"], s["new_coords"], s["vol"])
    ref32, hits = sc.ref_voxel_query(s, max_range, nsample, sc.d2_f32)
    ref64, _ = sc.ref_voxel_query(s, max_range, nsample, sc.d2_f64)
    assert np.array_equal(got, ref32)
    if family == "lattice":
        assert np.array_equal(ref32, ref64)
        if radius <= 2 and max_range[1] >= 1 and max_range[2] >= 1:
            for b, q in enumerate(s["planted"]):
                pz, py, px = sc.PLANT_VOXEL
                at, inside, outside = s["vol"][b, pz, py, px + 1], s["vol"][b, pz, py + 1, px], s["vol"][b, pz, py, px - 1]
                d = sc.d2_f64(s["new_xyz"][q:q + 1], s["xyz"][[at, inside, outside]])[0]
                assert d[0] == float(sc.r2_of(radius)) and d[1] < d[0] < d[2]
                members = set(sc._neighbourhood(s, q, max_range)[sc.d2_f64(s["new_xyz"][q:q + 1], s["xyz"][sc._neighbourhood(s, q, max_range)])[0]
                                                                  <= float(sc.r2_of(radius))].tolist())
                assert at in members and inside in members and outside not in members      # d2 == r2 is accepted here
    else:
        _check_float64(ref32, ref64, sc.ambiguous_voxel(s, max_range))
    # a batch index other than 0 matters: the same query coordinates against sample 0's volume give another answer
    assert (s["new_coords"][:, 0] > 0).any()


def test_voxel_cases_cover_what_they_claim():
    over, empty, border = 0, 0, 0
    Z, Y, X = sc.GRID
    for family, max_range, radius, nsample in sc.VOXEL_CASES:
        s = sc.voxel_scene(family, radius)
        _, hits = sc.ref_voxel_query(s, max_range, nsample, sc.d2_f32)
        over += int((hits > nsample).sum())
        empty += int((hits == 0).sum())
        zyx = s["new_coords"][:, 1:]
        border += int(((zyx == 0) | (zyx == np.array([Z - 1, Y - 1, X - 1]))).all(1).sum())      # corner queries
    assert over > 100 and empty > 100 and border >= 8 * 3 * len(sc.VOXEL_CASES)
    assert {n for _, _, _, n in sc.VOXEL_CASES} == set(sc.NSAMPLES)
    assert any(r[2] > X for _, r, _, _ in sc.VOXEL_CASES) and any(r[0] > Z for _, r, _, _ in sc.VOXEL_CASES) and any(r == (0, 0, 0) for _, r, _, _ in sc.VOXEL_CASES)


def test_gradient_cases_have_rows_with_many_contributions():
    """The (k + 2) bound is exercised: over the gradient cases some row collects thousands of contributions (a one-point sample that is
    every query's nearest; a clump of queries sharing their neighbours), not just k = 1."""
    most = 0
    for layout, family, channels in sc.INTERP_CASES:
        c = sc.cloud_case(layout, family)
        most = max(most, int(np.bincount(sc.ref_three_nn(c, sc.d2_f32)[1].reshape(-1)).max()))
    assert most >= 600
    most = 0
    for layout, family, radius, nsample, channels in sc.GROUP_CASES:
        c = sc.cloud_case(layout, family, radius)
        raw, _ = sc.ref_ball_query(c, nsample, sc.d2_f32)
        most = max(most, int(np.bincount(sc.global_rows(c, np.where(raw[:, :1] == -1, 0, raw)).reshape(-1)).max()))
    assert most >= 2000
