"""The builder and the restatement of tests/link_ref.py against the C oracle, on the CPU: every case of tests/test_gpu_link_edges.py sits
on the edge it was built for before the device sees it -- the designed increments / unique keys / edges of a first site are what
itertools.combinations gives, and what the oracle counts; the r2 / D' replay in Python floats gives the oracle's rows."""
import numpy as np
import pytest

from tests import link_ref as lr
from tests import util

TOL = 1e-6


@pytest.fixture(scope="module")
def lut():
    return util.load_lut()


def _agree(w, lut, min_snp=20, min_rows=0):
    """restatement == oracle on the counts; every position that holds observations is a called site; replay == oracle rows"""
    r = lr.restate(w)
    e = lr.expected(w, lut[0], lut[1], min_snp=min_snp)
    assert (r["n_increments"], r["n_edges"]) == (e["n_increments"], e["n_edges"])
    called = np.unique(e["snv"]["pos"][e["snv"]["allele_count"] >= 2])
    assert r["n_sites"] == len(called) == w["K"] and r["n_sites"] == len(np.unique(w["gpos"]))
    ld = e["ld"]
    assert len(ld) >= min_rows
    r2, dp = lr.replay_rows(ld["cAB"], ld["cAb"], ld["caB"], ld["cab"])
    for a, b in ((r2, ld["r2"]), (dp, ld["d_prime"])):
        assert np.array_equal(np.isnan(a), np.isnan(b))
        m = ~np.isnan(a)
        assert not m.any() or np.max(np.abs(a[m] - b[m])) <= TOL
    return r, e


@pytest.mark.parametrize("M,edges", [(1, 774), (8, 109)])
def test_ladder_sits_on_its_bucket_sizes(lut, M, edges):
    """family A: first site i has exactly the increments and unique keys of plan i, and nothing spills into another site's bucket"""
    w = lr.ladder(M).arrays()
    assert len(w["gpos"]) == 32778 and w["K"] == 223
    r, e = _agree(w, lut)
    assert r["n_increments"] == 9699 and r["n_edges"] == edges and r["n_allele_obs"] == 32778
    for i, (n, u) in enumerate(lr.LADDER):
        assert lr.site_shape(r, i) == (n, u, -(-u // (4 * M)))
    assert len(r["per_site"]) == len(lr.LADDER)
    rows = {20: (27, 428), 1: (770, 771)}
    for min_snp in (20, 1):
        ld = lr.expected(w, lut[0], lut[1], min_snp=min_snp)["ld"]
        assert len(ld) == rows[min_snp][M == 8]
        if min_snp == 1:
            assert int(np.isnan(ld["r2"]).sum()) == (5, 4)[M == 8] and len(ld) >= 700


def test_ladder_variants(lut):
    """the flush of one site's own edges, the plans that fall back by themselves, the reduced ladder of ISX_LINK_MAXU=40"""
    w = lr.ladder(1, edge_first=300, extra=320).arrays()
    r, _ = _agree(w, lut)
    assert lr.site_shape(r, len(lr.LADDER)) == (300, 300, 300)
    assert sum(lr.site_shape(r, i)[2] for i in range(16, 23)) > 256           # one round of a wave stages more than a flush holds
    for M in (1, 8):
        w = lr.ladder(M, plans=lr.LADDER + lr.FALLBACK, extra=240).arrays()
        r, _ = _agree(w, lut)
        assert [lr.site_shape(r, len(lr.LADDER) + i)[:2] for i in range(2)] == lr.FALLBACK
        assert max(v[1] for v in r["per_site"].values()) == 900 and sorted(v[1] for v in r["per_site"].values())[-3] == 768
    w = lr.ladder(1, plans=lr.REDUCED, extra=30).arrays()
    r, _ = _agree(w, lut)
    assert [lr.site_shape(r, i)[:2] for i in range(len(lr.REDUCED))] == lr.REDUCED and max(u for _, u in lr.REDUCED) == 40


@pytest.mark.parametrize("K", [4095, 4096, 4097, 4098, 8193])
def test_scan_cases_put_counts_on_the_tile_edges(lut, K):
    """family B: 25 increments at each listed rank, every one of them a row at min_snp 20"""
    w = lr.scan_case(K).arrays()
    r, e = _agree(w, lut, min_rows=1)
    firsts = lr.scan_firsts(K)
    assert {k for k in (4095, 4096, K - 2) if k <= K - 2} <= set(firsts)
    assert sorted(r["per_site"]) == [(0, lr.site_pos(k)) for k in firsts]
    assert all(v == (25, 4, 1) for v in r["per_site"].values()) and len(e["ld"]) == len(firsts)
    if K == 8193:
        assert len(w["gpos"]) == 8193 * 12 + 2 * 25 * len(firsts)


def test_scan_case_with_every_site_a_first_site(lut):
    w = lr.scan_case(4097, every=True).arrays()
    r, e = _agree(w, lut, min_snp=1, min_rows=4096)
    assert len(r["per_site"]) == 4096 and all(v == (3, 3, 1) for v in r["per_site"].values())


def test_pair_chain_cases(lut):
    """family C"""
    w = lr.long_pairs().arrays()
    r, e = _agree(w, lut)
    assert (len(w["gpos"]), r["n_increments"], r["n_edges"], len(e["ld"])) == (10400, 156000, 780, 6240)
    assert lr.site_shape(r, 0) == (200 * 39, 702, 39) and max(v[1] for v in r["per_site"].values()) == 702          # within LK_MAXU = 768
    w = lr.long_pairs(independent=True).arrays()
    r, e = _agree(w, lut)
    assert (r["n_increments"], r["n_edges"], len(e["ld"])) == (156000, 780, 6240) and lr.site_shape(r, 0)[1] > 768
    w = lr.self_pairs().arrays()
    r, e = _agree(w, lut, min_snp=1)
    k = r["keys"]
    p3, p4, p5, p6 = (lr.site_pos(i) for i in (3, 4, 5, 6))
    assert k[(0, p3, p3, 0, 0, 1)] == 3 and k[(0, p3, p3, 0, 1, 0)] == 3                       # the orientation is arrival order
    assert k[(0, p4, p4, 0, 0, 0)] == 3 and k[(0, p4, p4, 0, 0, 1)] == 6                       # three self increments a pair
    assert k[(0, p5, p5, 0, 0, 1)] == 3 and k[(0, p6, p6, 0, 1, 0)] == 3 and sum(c for q, c in k.items() if q[1] == p5 and q[2] == p6) == 12
    b, ids, logH, trio = lr.hashed_case()
    w = b.arrays(pair_ids=ids)
    r, _ = _agree(w, lut, min_snp=1)
    assert r["n_allele_obs"] == len(w["gpos"]) and (1 << logH) >= 2 * r["n_allele_obs"] and (logH == 12 or (1 << (logH - 1)) < 2 * r["n_allele_obs"])
    assert ids.min() == 0 and ids.max() == 2**32 - 2 and np.sort(ids)[1] > (1 << 20) + 8 * r["n_allele_obs"]
    assert len(set(lr.pair_hash(ids[list(trio)], logH).tolist())) == 1
    rd = lr.restate(b.arrays())
    assert rd["keys"] == r["keys"]
    w = lr.wave_case().arrays()
    r, _ = _agree(w, lut)
    assert all(c % 64 == 0 for c in np.bincount(w["gpos"])[lr.SITE0::lr.STEP])
    assert lr.site_shape(r, 0) == (65, 5, 2) and lr.site_shape(r, 1)[0] == 33 and lr.site_shape(r, 63) == (1, 1, 1)


def test_split_level_gate_and_tile_cases(lut):
    """families D - G: the restatement counts per split what the oracle counts per split"""
    b = lr.ladder(1)
    w = b.arrays(split_bounds=lr.split_bounds_for(b))
    r, _ = _agree(w, lut)
    assert r["n_increments"] < 9699 and (1, lr.site_pos(6)) not in r["per_site"]
    assert 0 < lr.site_shape(r, 4)[0] < 16                                                     # some of site 4's second sites lie behind the bound
    b, sb = lr.many_splits_case()
    r, _ = _agree(b.arrays(split_bounds=sb), lut, min_snp=1, min_rows=50)
    assert 0 < r["n_increments"] < 3 * 2099
    for M in (8, 128):
        w = lr.level_case(M).arrays()
        r, e = _agree(w, lut, min_rows=8)
        assert sorted(set(e["ld"]["mm"].tolist())) == sorted({0, M // 2 - 1, M // 2, M - 1, 3, 5})
    w = lr.gate_case().arrays()
    r, e = _agree(w, lut)
    ld = e["ld"]
    pa = ld["pos_a"].tolist()
    assert lr.site_pos(0) not in pa and lr.site_pos(2) in pa                                  # a table of 20 is no row, one of 21 is
    assert np.isnan(ld["r2"][ld["pos_a"] == lr.site_pos(12)]).all() and np.isnan(ld["d_prime"][ld["pos_a"] == lr.site_pos(14)]).all()
    assert (ld["pos_a"] == lr.site_pos(12)).sum() == 1 and (ld["pos_a"] == lr.site_pos(14)).sum() == 1
    b, sb = lr.dense_tile_case()
    w = b.arrays(split_bounds=sb)
    r, _ = _agree(w, lut, min_snp=1, min_rows=200)
    split = np.searchsorted(w["split_bounds"], w["gpos"], side="right") - 1
    assert [len(np.unique(w["gpos"][split == j])) for j in range(len(sb) - 1)] == lr.DENSE_SPLIT_SITES
    assert [len(np.unique(w["pair"][split == j])) for j in (9, 10, 11)] == [127, 128, 129]
