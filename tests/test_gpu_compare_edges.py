"""GPU: the per-pair compare body (isx_summary.hip run_compare: k_overlap_reduce / k_present_dense / k_level_apply, k_snv_keys /
k_snp_candidates / k_snp_apply / k_pack_compare, behind compare.calc_mm2overlap and compare.compare_scaffolds) at its edges.

Coverage half: against tests/summary_ref.py pair_levels (np.bincount of the observations; pinned on the host by tests/test_summary_ref.py)
on the tile-edge layout of tests/test_gpu_summary_edges.py, with samples of different numbers of levels, min_cov 1, 5 and 8 and
hand-placed positions at exactly min_cov - 1 and min_cov.

SNV half: hand-built piles of every kind the reference's rules tell apart, in a flat space of 200 000 positions (the sort keys use
bits above 32), expected rows from the CPU oracle per scaffold and oracle/compare.py.  Every hand-built position also carries the
verdict worked out by hand, and the oracle must agree with it -- a construction mistake cannot quietly empty a case.  Nothing expected
is read back from the device."""
import ctypes as C
import functools

import numpy as np
import pytest

from instrain_amd import _lib, compare, engine
from tests import summary_ref as sr, util
from tests.test_gpu_rollup_edges import _reads
from tests.test_gpu_summary_edges import _bases, _sorted, _tile_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    lut, fb = util.load_lut()
    c.set_null_model(lut, fb)
    yield c
    c.close()


def _batch(ctx, codes, bounds, obs, M):
    gpos, base, mm, pair = obs
    b = engine.Batch(ctx, codes, bounds, engine.pack_obs(gpos.astype(np.uint32), base, mm), pair, n_mm_bins=M, enable_linkage=False)
    b.run()
    return b


def _with_piles(obs, piles):
    """replace what a sample shows at the positions of `piles` {flat position: [(base, mm, count), ...]} by single-position reads"""
    gpos, base, mm, pair = obs
    keep = ~np.isin(gpos, np.fromiter(piles.keys(), dtype=np.int64, count=len(piles)))
    g = [gpos[keep]] + [np.full(n, p, dtype=np.int64) for p, lst in piles.items() for _, _, n in lst]
    b = [base[keep]] + [np.full(n, c, dtype=np.uint8) for lst in piles.values() for c, _, n in lst]
    m = [mm[keep]] + [np.full(n, lv, dtype=np.int64) for lst in piles.values() for _, lv, n in lst]
    g, b, m = np.concatenate(g), np.concatenate(b), np.concatenate(m)
    extra = len(g) - int(keep.sum())
    p = np.r_[pair[keep].astype(np.int64), int(pair.max()) + 1 + np.arange(extra)]
    return _sorted(g, b, m, p)


# ---- a. the coverage half ----
HAND = [70, 127, 128, 200, 5100, 16383, 16384, 20005, 31999]           # in seven lanes' tiles, both sides of a tile edge and of 16 384


def _raw_coverage(b1, b2, bounds, min_cov):
    out = np.zeros((len(bounds) - 1, max(b1.n_mm_bins, b2.n_mm_bins)), dtype=_lib.COMPARE_LEVEL_DT)
    ms = C.c_float(0)
    _lib.check(b1.lib.isx_compare_coverage(b1.h, b2.h, len(bounds) - 1, bounds.ctypes.data, int(min_cov), out.ctypes.data, C.byref(ms)))
    return out


@functools.lru_cache(maxsize=None)
def _coverage_sample(which, M, min_cov):
    """the tile-edge layout with reads of its own seed, and at the HAND positions coverage exactly: (A, B) = (min_cov - 1, min_cov),
    (min_cov, min_cov - 1), (min_cov, min_cov), (min_cov - 1, min_cov - 1), and min_cov reached only at the sample's LAST level
    (min_cov - 1 at level 0, one more read at level M - 1) in A, in B, in both -- cycling over the positions"""
    bounds, _, _, _, _, codes, _, empty = _tile_case(1, "on", False)
    rng = np.random.Generator(np.random.PCG64(7000 + 100 * which + 10 * M + min_cov))
    gpos, mm, pair = _reads(rng, bounds, 4, M, skip=empty)
    base = _bases(rng, gpos, codes)
    plan = [(-1, 0), (0, -1), (0, 0), (-1, -1), ("late", 0), (0, "late"), ("late", "late")]
    piles = {}
    for i, p in enumerate(HAND):
        want = plan[i % len(plan)][which]
        if want == "late":
            piles[p] = [(0, 0, min_cov - 1), (1, M - 1, 1)]
        else:
            piles[p] = [(0, 0, min_cov + want)]
    return _with_piles((gpos, base, mm, pair), piles), plan


@pytest.mark.parametrize("min_cov", [1, 5, 8])
@pytest.mark.parametrize("levels", [(1, 4), (3, 6), (6, 3)])
def test_overlap_tile_edges_levels_and_min_cov(ctx, levels, min_cov):
    """k_overlap_reduce on the tile-edge layout (scaffold ends on 63 .. 65 and 127 .. 129, scaffolds of 1, 2, 3, 1, 1 positions inside
    one tile, a bound exactly on 16 384, scaffolds without reads, n_pos = 2 * 16 384 + 1) for a dense sample against four levels, three
    against six and six against three levels (one sample's coverage carries over while the other's still grows), min_cov 1, 5 and 8,
    and positions where A, B or both have exactly min_cov - 1 or min_cov, or reach min_cov only at their last level.  both, either,
    present_a and present_b of every (scaffold, level) equal summary_ref.pair_levels; calc_mm2overlap's key sets are the union of
    presence and its coverage is both / either as the same float64 division, 0 when either is 0."""
    Ma, Mb = levels
    bounds = _tile_case(1, "on", False)[0]
    codes = _tile_case(1, "on", False)[5]
    n_pos = int(bounds[-1])
    (obs_a, plan), (obs_b, _) = _coverage_sample(0, Ma, min_cov), _coverage_sample(1, Mb, min_cov)
    ca, cb = sr.cov_levels(*obs_a[:3], n_pos, Ma), sr.cov_levels(*obs_b[:3], n_pos, Mb)
    for i, p in enumerate(HAND):                                         # the input really has the planned coverages
        for cov, M, want in ((ca, Ma, plan[i % len(plan)][0]), (cb, Mb, plan[i % len(plan)][1])):
            if want == "late":
                assert cov[-1, p] == min_cov and (M == 1 or (cov[:-1, p] == min_cov - 1).all())
            else:
                assert (cov[:, p] == min_cov + want).all()
    exp = sr.pair_levels(ca, cb, sr.presence(*obs_a[:3], bounds, Ma), sr.presence(*obs_b[:3], bounds, Mb), bounds, min_cov)
    A, B = _batch(ctx, codes, bounds, obs_a, Ma), _batch(ctx, codes, bounds, obs_b, Mb)
    raw = _raw_coverage(A, B, bounds, min_cov)
    mm2overlap, mm2coverage, ms = compare.calc_mm2overlap(A, B, bounds, min_cov=min_cov)
    raw2 = _raw_coverage(A, B, bounds, min_cov)
    A.close(); B.close()
    assert raw.tobytes() == raw2.tobytes() and ms > 0
    for f in ("both", "either"):
        assert (raw[f] == exp[f]).all(), (f, np.argwhere(raw[f] != exp[f])[:5])
    for f in ("present_a", "present_b"):
        assert ((raw[f] != 0) == exp[f]).all(), (f, np.argwhere((raw[f] != 0) != exp[f])[:5])
    assert (raw["consensus_snps"] == -1).all() and (raw["mm"] == np.arange(max(Ma, Mb))[None, :]).all()
    eo, ec = sr.overlap_dicts(exp)
    assert mm2overlap == eo and mm2coverage == ec
    assert not exp["present_a"][:, Ma:].any() and not exp["present_b"][:, Mb:].any() and exp["both"][:, -1].sum() > 20
    assert mm2overlap[0] == {} and mm2overlap[-1] == {}                  # no read, no key
    if min_cov > 4:                                                      # the one-position scaffold: four reads in either sample
        top = max(mm2overlap[1])                                         # (it may lack a level)
        assert exp["either"][1, -1] == 0 and mm2coverage[1][top] == 0 and mm2overlap[1][top] == 0


# ---- b. the SNV half ----
# A pile is what one sample shows at a position: [(base, level, reads)] with the bases R (the reference base there; base 0 at an N),
# X, Y, Z = the next three.  A kind = (name, pile of A, pile of B, verdict at min_freq 0.05, verdict at 0.1); a verdict is
# (consensus_SNP, population_SNP) or None: no mismatch row.  The null model has lut[18] = lut[20] = lut[40] = 2, lut[30] = 3.
R, X, Y, Z = 0, 1, 2, 3
REF = [(R, 0, 12)]                                                      # the reference base only: no SNV row
KINDS = [
    ("shared, equal consensus",                      [(X, 0, 12)], [(X, 0, 12)], None, None),
    ("(i) B shows A's consensus at the limit 3/30",  [(X, 0, 20)], [(Y, 0, 27), (X, 0, 3)], (True, False), (True, False)),
    ("(ii) one read below: 2/30",                    [(X, 0, 20)], [(Y, 0, 28), (X, 0, 2)], (True, True), (True, True)),
    ("A shows B's consensus at the limit 3/30",      [(Y, 0, 27), (X, 0, 3)], [(X, 0, 20)], (True, False), (True, False)),
    ("count / total == 0.05: 2/40",                  [(X, 0, 20)], [(Y, 0, 38), (X, 0, 2)], (True, False), (True, True)),
    ("one read below 0.05: 1/40",                    [(X, 0, 20)], [(Y, 0, 39), (X, 0, 1)], (True, True), (True, True)),
    ("count / total == 0.1: 4/40",                   [(X, 0, 20)], [(Y, 0, 36), (X, 0, 4)], (True, False), (True, False)),
    ("one read below 0.1: 3/40",                     [(X, 0, 20)], [(Y, 0, 37), (X, 0, 3)], (True, False), (True, True)),
    ("(iii) both multi-allelic, same var_base",      [(X, 0, 12), (Z, 0, 6)], [(Y, 0, 12), (Z, 0, 6)], (True, False), (True, False)),
    ("both multi-allelic, other var_base",           [(X, 0, 12), (Z, 0, 6)], [(Y, 0, 12), (R, 0, 6)], (True, True), (True, True)),
    ("(iv) population SNP",                          [(X, 0, 20)], [(Y, 0, 20)], (True, True), (True, True)),
    ("only A, reference present",                    [(X, 0, 12), (R, 0, 6)], REF, (True, False), (True, False)),
    ("only A, reference absent",                     [(X, 0, 18)], REF, (True, True), (True, True)),
    ("only A, consensus is the reference",           [(R, 0, 12), (X, 0, 6)], REF, None, None),
    ("only A, reference at the limit 3/30",          [(X, 0, 27), (R, 0, 3)], REF, (True, False), (True, False)),
    ("only A, reference one below: 2/30",            [(X, 0, 28), (R, 0, 2)], REF, (True, True), (True, True)),
    ("only B, reference present",                    REF, [(X, 0, 12), (R, 0, 6)], (True, False), (True, False)),
    ("only B, reference absent",                     REF, [(X, 0, 18)], (True, True), (True, True)),
    # rows at several levels: the row of the highest level decides, whatever the lower ones say
    ("two levels in A: SNS at 0, the reference wins at 2", [(X, 0, 10), (R, 2, 15)], REF, None, None),
    ("two levels in A: reference at 0, SNS wins at 1",     [(R, 0, 6), (X, 0, 5), (X, 1, 20)], REF, (True, False), (True, False)),
    ("three levels in A, two in B: agree at the top",      [(X, 0, 10), (Y, 1, 12), (X, 2, 14)], [(Y, 0, 10), (X, 2, 15)], None, None),
    ("three levels in A, two in B: differ at the top",     [(Y, 0, 10), (X, 1, 12), (Y, 2, 14)], [(Y, 0, 10), (X, 2, 15)], (True, False), (True, False)),
    ("two levels in both: equal below, differ at the top, same var_base", [(X, 0, 10), (Y, 1, 30)], [(X, 0, 10), (Z, 2, 30)],
     (True, False), (True, False)),
]
# totals around the null model's table (10 001 entries, lut[8578] and lut[10000] hold the "no value" mark): one below its length, exactly
# at it, and on a "no value" entry.  At such depth min_freq >= 0.05 asks for far more reads than any table value or the fallback, so the
# verdicts follow from the frequencies alone -- as long as the lookup's range check holds.
DEEP = [
    ("totals 10 000 and 10 001: 600 reads of the other's consensus", [(X, 0, 9400), (Y, 0, 600)], [(Y, 0, 9401), (X, 0, 600)],
     (True, False), (True, True)),
    ("total 8 578 ('no value'), one-sided, 578 reference reads",    [(X, 0, 8000), (R, 0, 578)], REF, (True, False), (True, True)),
]
N_ROW = ("one-sided row at an N reference base", [(X, 0, 12)], [(4, 0, 12)], "fails", "fails")
N_SHARED = ("shared row at an N reference base", [(X, 0, 12)], [(Y, 0, 12)], (True, True), (True, True))
SNV_BOUNDS = np.array([0, 50000, 70001, 140000, 200000], dtype=np.int64)
MA, MB = 3, 4


@functools.lru_cache(maxsize=None)
def _snv_case():
    """-> bounds, codes, seq, observations of A and B, and the hand-built sites [(flat position, scaffold, kind)]"""
    bounds = SNV_BOUNDS
    n_pos = int(bounds[-1])
    rng = np.random.Generator(np.random.PCG64(20000))
    codes = rng.integers(0, 4, n_pos).astype(np.uint8)
    lut, _ = util.load_lut()
    assert len(lut) == 10001 and lut[8578] < 0 and lut[10000] < 0 and lut[9999] >= 0 and [int(lut[t]) for t in (18, 20, 30, 40)] == [2, 2, 3, 2]
    # where: every kind in scaffolds 0 and 2; the scaffolds' first and last positions (flat 0 and n_pos - 1 among them) taken by hand
    sites = []
    fixed = {0: KINDS[10], 49999: KINDS[12], 50000: KINDS[1], 70000: KINDS[17], 70001: KINDS[2], 139999: KINDS[11], 140000: KINDS[16],
             n_pos - 1: KINDS[10]}
    taken = set(fixed)
    def free(s, n):
        got = []
        while len(got) < n:
            p = int(rng.integers(bounds[s] + 1, bounds[s + 1] - 1))
            if p not in taken:
                taken.add(p)
                got.append(p)
        return got
    for s in (0, 2):
        sites += [(p, s, k) for p, k in zip(free(s, len(KINDS) + len(DEEP)), KINDS + DEEP)]
    sites += [(p, 1, k) for p, k in zip(free(1, 5), [N_ROW, KINDS[10], KINDS[11], KINDS[0], KINDS[8]])]
    sites += [(p, 3, k) for p, k in zip(free(3, 5), [N_SHARED, KINDS[4], KINDS[7], KINDS[19], KINDS[21]])]
    sites += [(p, int(np.searchsorted(bounds, p, side="right") - 1), k) for p, k in fixed.items()]
    for p, s, k in sites:
        if k in (N_ROW, N_SHARED):
            codes[p] = 4
    # the background: depth 10, reference bases; and 150 random sites where a sample shows another base in part of its reads
    obs = []
    noisy = np.array(free(0, 40) + free(1, 30) + free(2, 40) + free(3, 40))
    for which, M in ((0, MA), (1, MB)):
        gpos, mm, pair = _reads(rng, bounds, 10, M)
        base = codes[gpos].copy()
        for p in noisy[rng.random(len(noisy)) < 0.7]:
            at = np.flatnonzero(gpos == p)
            base[at[rng.random(len(at)) < rng.choice([0.3, 0.5, 0.9])]] = (codes[p] + rng.integers(1, 4)) % 4
        piles = {}
        for p, s, k in sites:
            r = 0 if codes[p] == 4 else int(codes[p])
            piles[p] = [((c + r) % 4 if c < 4 else 4, lv, n) for c, lv, n in k[1 + which]]
        obs.append(_with_piles((gpos, base, mm, pair), piles))
    return bounds, codes, "".join(np.array(list("ACTGN"))[codes]), obs[0], obs[1], sites


@functools.lru_cache(maxsize=None)
def _snv_expected(min_freq):
    """oracle.profile_split per scaffold and sample (CPU), then oracle/compare.py: the route of
    tests/test_gpu_compare.py::test_snp_compare_multi_scaffold_vs_oracle; `except KeyError` is the reference's own N failure"""
    from oracle import compare as ocompare, oracle
    lut, fb = util.load_lut()
    bounds, codes, seq, obs_a, obs_b, sites = _snv_case()
    exp_rows, exp_table, snv_at = [], [], {}
    for i, (s, e) in enumerate(zip(bounds[:-1], bounds[1:])):
        def split(o):
            k = (o[0] >= s) & (o[0] < e)
            return oracle.profile_split(o[0][k] - s, o[1][k], o[2][k], o[3][k].astype(np.int64), seq[s:e], 0, lut, fb)
        ra, rb = split(obs_a), split(obs_b)
        snv_at[i] = (set(ra["snv"]["pos"].tolist()), set(rb["snv"]["pos"].tolist()))
        o, c = ocompare.calc_mm2overlap(ra["entries"], rb["entries"], int(e - s), min_cov=5)
        try:
            rows = ocompare.compare_snp_tables(ra["snv"], rb["snv"], o, lut, fb, min_freq=min_freq)
        except KeyError:
            exp_table.append((i, None, None, None, None, None, None))
            continue
        exp_rows += [(i, mm, p, cc, q) for mm, p, cc, q in rows]
        for t in ocompare.overlap_table(o, c, rows, int(e - s)):
            exp_table.append((i, t["mm"], t["compared_bases_count"], t["consensus_SNPs"], t["population_SNPs"], t["conANI"], t["popANI"]))
    return exp_rows, exp_table, snv_at


def _sorted_raw(raw):
    return raw[np.lexsort((raw["gpos"], raw["mm"]))]


def _checked_expectation(min_freq):
    """the oracle's rows and table, after checking the construction: every hand-built position gives the verdict worked out by hand
    (the same at every level it is compared at) and has an SNV row in exactly the samples it should; every kind occurs"""
    bounds, codes, seq, obs_a, obs_b, sites = _snv_case()
    exp_rows, exp_table, snv_at = _snv_expected(min_freq)
    verdict = {}
    for i, mm, p, cc, q in exp_rows:
        assert verdict.setdefault((i, p), (cc, q)) == (cc, q)
    seen = set()
    for p, s, k in sites:
        want = k[3] if min_freq == 0.05 else k[4]
        rel = p - int(bounds[s])
        if s == 1:
            assert (s, rel) not in verdict                               # the failed scaffold has no rows at all
        else:
            assert verdict.get((s, rel)) == want, (k[0], p, verdict.get((s, rel)), want)
            seen.add(k[0])
        in_a, in_b = rel in snv_at[s][0], rel in snv_at[s][1]            # which sample has an SNV row there
        assert in_a == (k[1] is not REF) and in_b == (k[2] is not REF and k is not N_ROW), (k[0], p, in_a, in_b)
    assert seen == {k[0] for k in KINDS + DEEP} | {N_SHARED[0]}
    assert [t[0] for t in exp_table if t[1] is None] == [1] and len(exp_rows) > 150
    assert {(0, 0), (0, 49999), (2, 0), (2, 69998), (3, 0), (3, 59999)} <= set(verdict)
    return exp_rows, exp_table


@pytest.mark.parametrize("min_freq", [0.05, 0.1])
def test_snp_compare_every_kind_on_a_large_flat_space(ctx, min_freq):
    """k_snv_keys / k_snp_candidates / k_snp_apply / k_pack_compare on 200 000 positions in four scaffolds (gpos beyond 65 536 and
    131 072: the 48-bit sort keys use bits above 32), three levels against four, background depth 10.  Hand-built, in scaffolds 0 and
    2 each: a shared position with equal consensus; different consensus where (i) B shows A's consensus at exactly the is_present limit,
    (ii) one read below it, (iii) both are multi-allelic with the same var_base, (iv) none applies (a population SNP); count / total
    exactly min_freq (2/40 at 0.05, 4/40 at 0.1) and one read below; rows in A only and in B only with the reference base present,
    absent, at the limit (count == min_bases) and one below, and with con_base == ref_base; rows at two and three levels of one
    position in one sample and in both, where the highest level's row overturns the lower one's verdict; totals one below and exactly
    at the null model's length and on a 'no value' entry.  Scaffold 1 holds a one-sided row at an N reference base: it alone fails
    (-2 in its rows, its mismatch rows dropped), its neighbours do not; scaffold 3 holds a SHARED row at an N, which does not fail.
    Flat position 0, n_pos - 1 and every scaffold's first and last position carry a SNP (find_seg at the bounds).  Mismatch rows and
    table columns equal the oracle's exactly; a second call gives the same; with the batches swapped the counts are the same and the
    raw rows mirrored."""
    bounds, codes, seq, obs_a, obs_b, sites = _snv_case()
    n_pos = int(bounds[-1])
    exp_rows, exp_table = _checked_expectation(min_freq)
    A, B = _batch(ctx, codes, bounds, obs_a, MA), _batch(ctx, codes, bounds, obs_b, MB)
    table, mdb, ms = compare.compare_scaffolds(A, B, bounds, min_cov=5, min_freq=min_freq, store_mismatch_locations=True)
    table2, mdb2, _ = compare.compare_scaffolds(A, B, bounds, min_cov=5, min_freq=min_freq, store_mismatch_locations=True)
    table_s, mdb_s, _ = compare.compare_scaffolds(B, A, bounds, min_cov=5, min_freq=min_freq, store_mismatch_locations=True)
    A.close(); B.close()
    raw = _sorted_raw(mdb["raw"])
    assert ms > 0 and int(raw["gpos"].max()) == n_pos - 1 and int(raw["gpos"].min()) == 0
    got_rows = sorted(zip(mdb["scaffold"].tolist(), mdb["raw"]["mm"].tolist(), mdb["position"].tolist(),
                          mdb["raw"]["consensus_snp"].astype(bool).tolist(), mdb["raw"]["population_snp"].astype(bool).tolist()))
    assert got_rows == sorted(exp_rows)
    got_table = [(r["scaffold"], r.get("mm"), r.get("compared_bases_count"), r.get("consensus_SNPs"), r.get("population_SNPs"),
                  r.get("conANI"), r.get("popANI")) for r in table]
    assert len(got_table) == len(exp_table)
    for g, e in zip(got_table, exp_table):
        assert g[:5] == e[:5], (g, e)
        for x, y in zip(g[5:], e[5:]):
            assert x == y or (x is not None and np.isnan(x) and np.isnan(y)), (g, e)
    assert table[[t[0] for t in got_table].index(1)] == {"scaffold": 1, "failed": True} and not (mdb["scaffold"] == 1).any()
    # a second call (reused buffers) and the swapped pair
    assert len(table2) == len(table) and all(str(a) == str(b) for a, b in zip(table, table2))
    assert _sorted_raw(mdb2["raw"]).tobytes() == raw.tobytes()
    key = lambda r: (r.get("scaffold"), r.get("mm"), r.get("compared_bases_count"), r.get("consensus_SNPs"), r.get("population_SNPs"),
                     r.get("failed"))
    assert [key(r) for r in table_s] == [key(r) for r in table]
    swapped = _sorted_raw(mdb_s["raw"])
    assert len(swapped) == len(raw)
    for f in ("gpos", "mm", "consensus_snp", "population_snp"):
        assert (swapped[f] == raw[f]).all(), f
    for f in ("has_%s", "con_%s", "ref_%s", "var_%s", "cnt_%s"):
        assert (swapped[f % "a"] == raw[f % "b"]).all() and (swapped[f % "b"] == raw[f % "a"]).all(), f
    assert (raw["has_a"] == 0).any() and (raw["has_b"] == 0).any() and ((raw["has_a"] == 1) & (raw["has_b"] == 1)).any()
