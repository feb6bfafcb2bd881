"""The linkage bucket chain (csrc/isx_linkage.hip) at its bucket, table and scan edges, on batches BUILT to sit there (tests/link_ref.py;
tests/test_link_ref.py checks the builder against the oracle on the CPU) instead of random draws that may or may not land on them.

Every case is checked four ways (`_check`):
  (a) against the C oracle per split: integers exact, r2 / D' within TOL (util.assert_same on canon_from_struct);
  (b) sizes() against the plain-Python restatement of the counting (itertools.combinations per pair and split);
  (c) link_chain() is the chain the case was built for (3 bucket, 1 sorted, 2 dense MFMA);
  (d) `ld` and `snv` byte-identical to the same batch under ISX_LINK_CHAIN=sorted (mode 2: `ld` byte-identical to the bucket chain);
and the batch is run twice on the same handle with the same bytes (epoch-tagged heads, reused tables).  On top of (a), r2 and D' of EVERY row
equal, bit for bit, a Python-float replay of the reference's operation order on the row's own counts: the kernel computes them in fp64 with
contraction off, each operation correctly rounded, so the derived bound is zero.

Families: A bucket ladder (k_site_edges: 1 / 2..16 / 17..64 / table; 64 / 65 and 768 / 769 unique keys; lk_flush in mid-round), B scan edges
(k_scan_u32: tile ends, scalar tail, carry), C pair chains (growth steps, self pairs, hashed heads, a wave's ballot), D splits, E level field,
F gates and ties of ld_edge_rows, G the dense MFMA path's tile edges.

Reference: calc_mm_SNV_linkage_network linkage.py:14-44, _iterator_ld_sites :78-131, _calc_ld_single :138-196."""
import numpy as np
import pytest

from tests import link_ref as lr
from tests import util

pytestmark = pytest.mark.gpu
TOL = 1e-6
_CASES, _EXP = {}, {}


@pytest.fixture(scope="module")
def ctx():
    from instrain_amd import engine
    lut, fb = util.load_lut()
    c = engine.Context(0)
    c.set_null_model(lut, fb)
    yield c
    c.close()


def _case(name, make):
    """(arrays, restatement) of a named case, built once"""
    if name not in _CASES:
        w = make()
        _CASES[name] = (w, lr.restate(w))
    return _CASES[name]


def _expected(name, w, min_snp):
    if (name, min_snp) not in _EXP:
        lut, fb = util.load_lut()
        _EXP[(name, min_snp)] = lr.expected(w, lut, fb, min_snp=min_snp)
    return _EXP[(name, min_snp)]


def _run(ctx, w, M, **kw):
    from instrain_amd import engine
    obs = engine.pack_obs(w["gpos"].astype(np.uint32), w["base"], w["mm"])
    b = engine.Batch(ctx, w["ref_codes"], w["split_bounds"], obs, w["pair"], n_mm_bins=M, enable_linkage=True, **kw)
    b.run()
    f, s, c = b.fetch(), b.sizes(), b.link_chain()
    b.run()                                     # the same batch again: the chain's tables are reused (epoch-tagged heads)
    f2, c2 = b.fetch(), b.link_chain()
    b.close()
    assert f["ld"].tobytes() == f2["ld"].tobytes() and f["snv"].tobytes() == f2["snv"].tobytes() and c == c2
    return f, s, c


def _check(ctx, monkeypatch, name, make, M, chain, min_snp=20, env=None, linkage_mode=0):
    from tests import prod
    w, r = _case(name, make)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    f, s, c = _run(ctx, w, M, min_snp=min_snp, linkage_mode=linkage_mode)
    for k in (env or {}):
        monkeypatch.delenv(k)
    assert c == chain, (name, "chain", c)                                                           # (c)
    exp = _expected(name, w, min_snp)                                                               # (a)
    got = prod.to_oracle_layout(f, lambda g: g.astype(np.int64))
    util.assert_same(util.canon_from_struct(got), util.canon_from_struct(exp), float_tol=TOL, what=name)
    for k in ("n_increments", "n_edges", "n_sites", "n_allele_obs"):                                # (b)
        assert s[k] == r[k], (name, k, s[k], r[k])
    assert s["n_ld"] == len(exp["ld"]) == len(f["ld"])
    ld = f["ld"]                                                                                    # the float rule: zero distance to the replay
    r2, dp = lr.replay_rows(ld["countAB"], ld["countAb"], ld["countaB"], ld["countab"])
    assert lr.same_bits(ld["r2"], r2), (name, "r2", np.nanmax(np.abs(ld["r2"] - r2)))
    assert lr.same_bits(ld["d_prime"], dp), (name, "d_prime", np.nanmax(np.abs(ld["d_prime"] - dp)))
    if linkage_mode == 2:                                                                           # (d)
        f2, s2, c2 = _run(ctx, w, M, min_snp=min_snp)
        assert c2 == 3
    else:
        monkeypatch.setenv("ISX_LINK_CHAIN", "sorted")
        f2, s2, c2 = _run(ctx, w, M, min_snp=min_snp)
        monkeypatch.delenv("ISX_LINK_CHAIN")
        assert c2 == 1
        assert f["snv"].tobytes() == f2["snv"].tobytes(), name
    assert f["ld"].tobytes() == f2["ld"].tobytes(), name
    for k in ("n_ld", "n_edges", "n_increments", "n_allele_obs", "n_snv", "n_sites"):
        assert s[k] == s2[k], (name, k, s[k], s2[k])
    return f, s, r, exp


# ---- A. bucket ladder -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("min_snp", [20, 1])
@pytest.mark.parametrize("M", [1, 8])
def test_bucket_ladder(ctx, monkeypatch, M, min_snp):
    """buckets of 1, 2, 15..17, 63..65, 128..5000 increments with 1..768 unique keys, one first site each; 768 is the last number of unique
    keys that stays on the bucket chain.  Listed sites 16..22 share a wave's round and stage 661 edges (M = 1): lk_flush runs in mid-round"""
    f, s, r, exp = _check(ctx, monkeypatch, "ladder%d" % M, lambda: lr.ladder(M).arrays(), M, 3, min_snp=min_snp)
    assert [lr.site_shape(r, i)[:2] for i in range(len(lr.LADDER))] == lr.LADDER
    assert (len(_CASES["ladder%d" % M][0]["gpos"]), s["n_sites"], s["n_increments"], s["n_edges"]) == (32778, 223, 9699, 774 if M == 1 else 109)
    assert len(f["ld"]) == {(1, 20): 27, (8, 20): 428, (1, 1): 770, (8, 1): 771}[(M, min_snp)]
    if min_snp == 1:
        assert len(f["ld"]) >= 700 and int(np.isnan(f["ld"]["r2"]).sum()) == (5 if M == 1 else 4)


def test_one_site_stages_more_edges_than_a_flush_holds(ctx, monkeypatch):
    """300 unique keys on 300 different second sites: a single site passes LK_STAGE staged edges on its own"""
    f, s, r, _ = _check(ctx, monkeypatch, "ladder_edge_first", lambda: lr.ladder(1, edge_first=300, extra=320).arrays(), 1, 3)
    assert lr.site_shape(r, len(lr.LADDER)) == (300, 300, 300) and s["n_edges"] == 774 + 300


@pytest.mark.parametrize("M", [1, 8])
def test_ladder_with_769_keys_falls_back_by_itself(ctx, monkeypatch, M):
    """(1000, 769) and (2000, 900) appended: the batch takes the sorted chain with no environment variable"""
    f, s, r, _ = _check(ctx, monkeypatch, "ladder_fb%d" % M, lambda: lr.ladder(M, plans=lr.LADDER + lr.FALLBACK, extra=240).arrays(), M, 1)
    assert sorted(v[1] for v in r["per_site"].values())[-3:] == [768, 769, 900] and len(f["ld"]) > 20


@pytest.mark.parametrize("max_u,chain", [(40, 3), (39, 1)])
def test_reduced_ladder_through_the_lds_table(ctx, monkeypatch, max_u, chain):
    """ISX_LINK_MAXU below 64: reg_max = 1, every bucket of two or more goes through the LDS table -- 64 slots for 2..32 increments, 128 for
    33..64, 256 for 65, 1024 for 512 and 513; 40 unique keys stay (lim = min(40, 48)), one fewer allowed sends the batch to the sorted chain"""
    f, s, r, _ = _check(ctx, monkeypatch, "reduced", lambda: lr.ladder(1, plans=lr.REDUCED, extra=30).arrays(), 1, chain, min_snp=1,
                        env={"ISX_LINK_MAXU": str(max_u)})
    assert [lr.site_shape(r, i)[:2] for i in range(len(lr.REDUCED))] == lr.REDUCED and len(f["ld"]) > 50


# ---- B. scan edges ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [4095, 4096, 4097, 4098, 8193])
def test_scan_edges(ctx, monkeypatch, K):
    """non-zero counts (increments, then rows) on the last element of a 4096-tile, the first of the next, in the scalar tail (K % 4 = 1, 2, 3)
    and behind a carry of two tiles"""
    f, s, r, _ = _check(ctx, monkeypatch, "scan%d" % K, lambda: lr.scan_case(K).arrays(), 1, 3)
    firsts = lr.scan_firsts(K)
    assert s["n_sites"] == K and len(f["ld"]) == len(firsts) and s["n_increments"] == 25 * len(firsts)
    assert f["ld"]["gpos_a"].tolist() == [lr.site_pos(k) for k in firsts]


def test_scan_with_every_site_a_first_site(ctx, monkeypatch):
    """the list of non-zero entries is the whole array (but its last element)"""
    f, s, r, _ = _check(ctx, monkeypatch, "scan_every", lambda: lr.scan_case(4097, every=True).arrays(), 1, 3, min_snp=1)
    assert s["n_edges"] == 4096 and len(f["ld"]) == 4096


# ---- C. pair chains ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("independent,chain", [(False, 3), (True, 1)])
def test_long_pairs_grow_both_tables(ctx, monkeypatch, independent, chain):
    """200 pairs over all 40 sites: 156 000 increments and 6 240 rows.  The chain's tables belong to the batch (isx_batch::L) and every run
    here makes a new batch, whose first attempt offers max(2 x allele observations, 65 536) = 65 536 keys and 4 096 rows: both are too
    small, so LKF_KEYS and LKF_LD re-enter the chain with no ISX_LINK_TEST_CAPS.  That the growth steps ran is inferred from those sizes
    in bucket_chain(), not observed -- no API reports it; what is observed is the right tables, and the same bytes from the second run
    on the grown tables.  Haplotype pairs keep site 0 at 702 unique keys (bucket chain); with every base drawn by itself it has 1 248:
    the key table grows and then LKF_BUCKET hands the ranked observations to the sorted chain"""
    f, s, r, _ = _check(ctx, monkeypatch, "long_pairs%d" % independent, lambda: lr.long_pairs(independent).arrays(), 8, chain)
    assert (s["n_allele_obs"], s["n_increments"], s["n_edges"], s["n_ld"]) == (10400, 156000, 780, 6240)
    assert (lr.site_shape(r, 0)[1] > 768) == independent


def test_three_site_pairs_and_self_pairs(ctx, monkeypatch):
    """a pair twice on one column as (A, C), another as (C, A): the orientation is arrival order; three times on a column: three self
    increments; two observations on each of two sites"""
    f, s, r, _ = _check(ctx, monkeypatch, "self_pairs", lambda: lr.self_pairs().arrays(), 1, 3, min_snp=1)
    ld = f["ld"]
    self_rows = ld[ld["gpos_a"] == ld["gpos_b"]]
    assert sorted(self_rows["gpos_a"].tolist()) == [lr.site_pos(k) for k in (3, 4, 5, 6)]
    row3 = self_rows[self_rows["gpos_a"] == lr.site_pos(3)][0]
    assert (int(row3["countAb"]), int(row3["countaB"])) == (3, 3)


def test_hashed_heads_with_two_pairs_on_one_slot(ctx, monkeypatch):
    """pair ids above 2^20 + 8 x allele observations (incl. 0 and 2^32 - 2): the heads are a hash table; three pairs computed to share a slot,
    two of them interleaved on the same two sites.  The same observations with dense ids give the same LD bytes"""
    b, ids, logH, trio = lr.hashed_case()
    f, s, r, _ = _check(ctx, monkeypatch, "hashed", lambda: b.arrays(pair_ids=ids), 1, 3, min_snp=1)
    assert (1 << logH) >= 2 * s["n_allele_obs"] and len(set(lr.pair_hash(ids[list(trio)], logH).tolist())) == 1
    fd, sd, _, _ = _check(ctx, monkeypatch, "hashed_dense_ids", lambda: b.arrays(), 1, 3, min_snp=1)
    assert f["ld"].tobytes() == fd["ld"].tobytes()


def test_wave_of_one_two_and_64_first_sites(ctx, monkeypatch):
    """64 side-by-side observations whose pairs' first sites are 1, 2 (32 + 32) and 64 different sites: one atomic, two, 64 in a walk step"""
    f, s, r, _ = _check(ctx, monkeypatch, "wave", lambda: lr.wave_case().arrays(), 1, 3)
    assert s["n_increments"] == 192 and lr.site_shape(r, 0) == (65, 5, 2)


# ---- D. splits --------------------------------------------------------------------------------------------------------------------------

def test_split_bounds_through_the_ladder(ctx, monkeypatch):
    """a bound between a first site and some of its second sites, one on a site's position, one past a site, a one-position split, two empty ones"""
    def make():
        b = lr.ladder(1)
        return b.arrays(split_bounds=lr.split_bounds_for(b))
    f, s, r, _ = _check(ctx, monkeypatch, "ladder_splits", make, 1, 3, min_snp=1)
    assert 0 < s["n_increments"] < 9699 and len(f["ld"]) > 50


def test_two_thousand_splits(ctx, monkeypatch):
    def make():
        b, sb = lr.many_splits_case()
        return b.arrays(split_bounds=sb)
    f, s, r, _ = _check(ctx, monkeypatch, "splits2000", make, 1, 3, min_snp=1)
    assert len(f["ld"]) > 50


# ---- E. level field ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", [8, 128])
def test_level_field(ctx, monkeypatch, M):
    """linking pairs at levels 0, M/2 - 1, M/2 and M - 1 (128 bins is the most isx_batch_create takes): the key's mm field, site_cum over
    every level; a site that holds a level only through pairs that do not reach the other site of an edge"""
    f, s, r, _ = _check(ctx, monkeypatch, "levels%d" % M, lambda: lr.level_case(M).arrays(), M, 3)
    assert sorted(set(f["ld"]["mm"].tolist())) == sorted({0, M // 2 - 1, M // 2, M - 1, 3, 5})


@pytest.mark.parametrize("M", [129, 256, 257])
def test_more_bins_than_the_batch_takes_are_refused(ctx, M):
    from instrain_amd import engine
    w = lr.level_case(8).arrays()
    with pytest.raises(engine.IsxError) as e:
        _run(ctx, w, M)
    assert e.value.code == -1                   # ISX_ERR_ARG


# ---- F. gates and ties of ld_edge_rows --------------------------------------------------------------------------------------------------

def test_gates_and_ties(ctx, monkeypatch):
    """pair tables of exactly 20 (no row) and 21 (a row) at min_snp 20; shallow columns whose two sites sum to 19 and 20; alleles tied at a site (A<C<T<G) and
    a third allele above threshold; one allele absent among the spanning pairs: r2 and D' NaN"""
    f, s, r, _ = _check(ctx, monkeypatch, "gates", lambda: lr.gate_case().arrays(), 1, 3)
    ld = f["ld"]
    pa = ld["gpos_a"].tolist()
    assert lr.site_pos(0) not in pa and ld[ld["gpos_a"] == lr.site_pos(2)]["total"].tolist() == [21]
    tie = ld[(ld["gpos_a"] == lr.site_pos(9)) & (ld["gpos_b"] == lr.site_pos(10))][0]
    assert (int(tie["allele_A"]), int(tie["allele_a"]), int(tie["allele_B"]), int(tie["allele_b"])) == (1, 2, 0, 1)
    for k in (12, 14):
        row = ld[ld["gpos_a"] == lr.site_pos(k)]
        assert len(row) == 1 and np.isnan(row["r2"][0]) and np.isnan(row["d_prime"][0])
    _check(ctx, monkeypatch, "gates", lambda: lr.gate_case().arrays(), 1, 3, min_snp=3)


# ---- G. dense MFMA path -----------------------------------------------------------------------------------------------------------------

def _dense_cases():
    def ladder_splits():
        b = lr.ladder(1)
        return b.arrays(split_bounds=lr.split_bounds_for(b))

    def tiles():
        b, sb = lr.dense_tile_case()
        return b.arrays(split_bounds=sb)

    def hashed():
        b, ids, _, _ = lr.hashed_case()
        return b.arrays(pair_ids=ids)
    def splits2000():
        b, sb = lr.many_splits_case()
        return b.arrays(split_bounds=sb)
    return {"ladder1": lambda: lr.ladder(1).arrays(), "ladder_edge_first": lambda: lr.ladder(1, edge_first=300, extra=320).arrays(),
            "self_pairs": lambda: lr.self_pairs().arrays(), "hashed": hashed, "wave": lambda: lr.wave_case().arrays(),
            "ladder_splits": ladder_splits, "splits2000": splits2000, "dense_tiles": tiles}


@pytest.mark.parametrize("name", ["ladder1", "ladder_edge_first", "self_pairs", "hashed", "wave", "ladder_splits", "splits2000", "dense_tiles"])
def test_dense_mfma_path(ctx, monkeypatch, name):
    """linkage_mode 2 on the M = 1 cases of A (the ladder, and with the 300-edge site), C (self pairs, hashed ids, the wave) and D (the cut
    ladder; 2 000 splits: the path's per-split host loop, its back-fill of first rows / sites over splits without any, the one-site
    splits it skips between real ones) -- the fallback ladders and the reduced ladder are the same buckets under an environment variable the
    path does not read, the long pairs are M = 8 -- and on its own tile edges: splits of 1 (skipped by the path), 2, 7, 8, 9, 31, 32, 33
    and 129 sites, 127 / 128 / 129 distinct (split, pair) rows, a cell of 2 in X: the oracle's tables, `ld` byte for byte the bucket chain's"""
    f, s, r, _ = _check(ctx, monkeypatch, name, _dense_cases()[name], 1, 2, min_snp=1, linkage_mode=2)
    assert len(f["ld"]) > (100 if name in ("ladder1", "dense_tiles") else 0)
