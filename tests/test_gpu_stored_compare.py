"""GPU: samples that enter a compare.SampleSet from their STORED profile (SampleSet.add_profile, isx_cmpset_add_profile) instead of a
resident batch.  Expected values never come from the code under test: they are the reference's golden files, the add_batch route
(which tests/test_gpu_compare_set.py pins) or plain numpy.  Everything compared is an integer or a float made by the identical host
expression: equality throughout."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pandas as pd
import pytest

from tests import stored_ref, util
from tests.test_gpu_compare_set import _batch, _mdb_rows, _same_rows

pytestmark = pytest.mark.gpu

LENGTHS = [1, 63, 64, 65, 127, 128, 129, 4096, 4097, 8193]      # those of test_gpu_compare_set.py and three tiles with a tail of one position
NAMES = ["sc%d" % i for i in range(len(LENGTHS))]
SB = np.r_[0, np.cumsum(LENGTHS)]


@pytest.fixture(scope="module")
def ctx():
    from instrain_amd import engine
    c = engine.Context(0)
    lut, fb = util.load_lut()
    c.set_null_model(lut, fb)
    yield c
    c.close()


def _ser(pos, val):
    return pd.Series(np.asarray(val, dtype=np.int64), index=np.asarray(pos, dtype=np.int64))


def _levels_of(st):
    st.compare(min_freq=0.05)
    return st.levels.tobytes()


# ---- 1. the reference's vectors through add_profile ----
@pytest.mark.parametrize("name", ["compare_a", "compare_b", "compare_c", "compare_d"])
def test_reference_vectors_through_add_profile(ctx, name):
    """the assertions of test_reference_vectors_through_the_set; the SNV table is what a resident batch calls (pinned elsewhere), covT is numpy's"""
    from instrain_amd import compare, engine
    g = util.load_case(name)
    codes = engine.encode_seq(str(g["seq"]))
    st = compare.SampleSet(ctx, ["scaffold"], [len(codes)], min_cov=5)
    for s in "ab":
        pos, base, mm = g[s + "_pos"], g[s + "_base"], g[s + "_mm"]
        b = _batch(ctx, codes, [0, len(codes)], pos, base, mm, int(mm.max()) + 1)
        table = stored_ref.snv_frame(b.fetch()["snv"], [0, len(codes)], ["scaffold"])
        b.close()
        st.add_profile(s, stored_ref.covT_from_obs(pos, base, mm, [0, len(codes)], ["scaffold"]), table)
        assert st.profile_device_ms > 0
    table = st.compare(min_freq=0.05)
    mdb = st.mismatch_locations("a", "b")
    st.close()
    assert [r["mm"] for r in table] == list(g["mm"])
    assert [r["compared_bases_count"] for r in table] == list(g["both"])
    assert [r["consensus_SNPs"] for r in table] == list(g["t_consensus_SNPs"])
    assert [r["population_SNPs"] for r in table] == list(g["t_population_SNPs"])
    for k in ("conANI", "popANI", "percent_genome_compared"):
        np.testing.assert_array_equal(np.array([r[k] for r in table], dtype=np.float64), g["t_" + k])
    np.testing.assert_array_equal(np.array([r["coverage_overlap"] for r in table]), g["coverage"])
    assert {(r["name1"], r["name2"], r["scaffold"]) for r in table} == {("a", "b", "scaffold")}
    raw = mdb["raw"]
    assert list(raw["mm"]) == list(g["m_mm"]) and list(mdb["position"]) == list(g["m_position"])
    assert list(raw["consensus_snp"].astype(bool)) == list(g["m_consensus_SNP"])
    assert list(raw["population_snp"].astype(bool)) == list(g["m_population_SNP"])


def test_the_reference_on_stored_inputs(ctx):
    """tests/golden/make_stored_compare_golden.py: the reference's compare_scaffold on stored-format inputs (different key sets, a key with an
    empty series, a scaffold one sample lacks, an SNV row whose mm is no covT key, an empty SNP table) -- its table and mismatch rows"""
    from instrain_amd import compare
    names, lengths, samples, covT, tables = stored_ref.load_stored_golden(os.path.join(util.GOLD, "stored_compare_inputs.npz"))
    gold_t = pd.read_csv(os.path.join(util.GOLD, "stored_compare_table.csv"), float_precision="round_trip")      # (the default parser may be an ulp off)
    gold_t = gold_t.sort_values(["scaffold", "name1", "name2", "mm"])
    gold_m = pd.read_csv(os.path.join(util.GOLD, "stored_compare_mdb.csv"))
    st = compare.SampleSet(ctx, names, lengths, min_cov=5)
    for s in samples:
        st.add_profile(s, covT[s], tables[s])
    logs = []
    table = st.compare(min_freq=0.05, logs=logs)
    assert not logs and len(table) == len(gold_t) == 18
    for r, (_, e) in zip(table, gold_t.iterrows()):
        for k in ("scaffold", "name1", "name2", "mm", "compared_bases_count", "length", "consensus_SNPs", "population_SNPs",
                  "coverage_overlap", "percent_genome_compared", "conANI", "popANI"):
            assert r[k] == e[k], (k, r, dict(e))
    got = []
    for a, b in itertools.combinations(samples, 2):
        m = st.mismatch_locations(a, b)
        got += [(names[sc], a, b, mm, p, bool(c), bool(q)) for sc, mm, p, c, q in
                zip(m["scaffold"].tolist(), m["raw"]["mm"].tolist(), m["position"].tolist(), m["raw"]["consensus_snp"].tolist(),
                    m["raw"]["population_snp"].tolist())]
    st.close()
    exp = sorted(zip(gold_m["scaffold"], gold_m["name1"], gold_m["name2"], gold_m["mm"], gold_m["position"],
                     gold_m["consensus_SNP"].astype(bool), gold_m["population_SNP"].astype(bool)))
    assert sorted(got) == exp and len(exp) > 20


# ---- 2. / 3. / 7. five samples: a set fed by add_profile against a set fed by add_batch ----
class Sample:
    """tests/test_gpu_compare_set.py's Sample over this file's LENGTHS: observations, `mm` = device levels, `values` their real mm"""

    def __init__(self, name, seed, depth, n_levels, values=None, drop=()):
        from tests.test_gpu_parity import _random_split
        self.name, self.n_levels = name, n_levels
        self.values = list(range(n_levels)) if values is None else list(values)
        _, pos, base, mm, _ = _random_split(seed, int(SB[-1]), depth, n_levels, 60)
        keep = np.ones(len(pos), bool)
        for sc in drop:
            keep &= ~((pos >= SB[sc]) & (pos < SB[sc + 1]))
        self.pos, self.base = pos[keep], base[keep]
        self.mm = (mm[keep] if n_levels > 1 else mm[keep] * 0).astype(np.int64)
        self.real_mm = np.asarray(self.values)[self.mm]
        self.table = None

    def batch(self, ctx, codes, scaffolds=None):
        """-> (a run batch of the observations on these scaffolds, in this order, as a flat space of their own; names; bounds)"""
        scaffolds = list(range(len(LENGTHS))) if scaffolds is None else list(scaffolds)
        bounds = np.r_[0, np.cumsum([LENGTHS[sc] for sc in scaffolds])]
        sel, new_pos = [], []
        for k, sc in enumerate(scaffolds):
            idx = np.flatnonzero((self.pos >= SB[sc]) & (self.pos < SB[sc + 1]))
            sel.append(idx)
            new_pos.append(self.pos[idx] - SB[sc] + bounds[k])
        sel, new_pos = np.concatenate(sel), np.concatenate(new_pos)
        ref = np.concatenate([codes[SB[sc]:SB[sc + 1]] for sc in scaffolds])
        return _batch(ctx, ref, bounds, new_pos, self.base[sel], self.mm[sel], self.n_levels), [NAMES[sc] for sc in scaffolds], bounds

    def covT(self, scaffolds=None):
        c = stored_ref.covT_from_obs(self.pos, self.base, self.real_mm, SB, NAMES)
        return c if scaffolds is None else {NAMES[sc]: c[NAMES[sc]] for sc in scaffolds if NAMES[sc] in c}

    def snv(self, scaffolds=None):
        t = self.table
        return t if scaffolds is None or len(t) == 0 else t[t["scaffold"].isin([NAMES[sc] for sc in scaffolds])]


def _results(st, samples):
    table = st.compare(min_freq=0.05)
    return table, st.levels.copy(), {(a.name, b.name): st.mismatch_locations(a.name, b.name) for a, b in itertools.combinations(samples, 2)}


@pytest.fixture(scope="module")
def five(ctx):
    """the five samples; the batch-fed set (the yardstick) and the profile-fed set, both left open"""
    from instrain_amd import compare, engine
    from tests.test_gpu_parity import _random_split
    seq = re.sub("[^ACGT]", "A", _random_split(700, int(SB[-1]), 5, 1, 10)[0])
    codes = engine.encode_seq(seq)
    samples = [Sample("s0", 701, 30, 1), Sample("s1", 702, 24, 1, drop=(3, 7)), Sample("s2", 703, 26, 4),
               Sample("s3", 704, 28, 3, values=[0, 1, 3]), Sample("s4", 705, 22, 2, values=[0, 2])]
    by_batch = compare.SampleSet(ctx, NAMES, LENGTHS, min_cov=5)
    for s in samples:
        b, names, bounds = s.batch(ctx, codes)
        by_batch.add_batch(s.name, b, names, bounds, mm_values=s.values)
        s.table = stored_ref.snv_frame(b.fetch()["snv"], SB, NAMES, mm_values=s.values)     # the sample's cumulative_snv_table
        b.close()
    by_profile = compare.SampleSet(ctx, NAMES, LENGTHS, min_cov=5)
    for s in samples:
        by_profile.add_profile(s.name, s.covT(), s.snv(), mm_values=s.values)
    out = dict(codes=codes, samples=samples, by_batch=by_batch, by_profile=by_profile)
    out["table"], out["levels"], out["mdbs"] = _results(by_batch, samples)
    yield out
    by_batch.close()
    by_profile.close()


def _assert_same_set(st, five):
    table, levels, mdbs = _results(st, five["samples"])
    assert levels.tobytes() == five["levels"].tobytes()
    _same_rows(table, five["table"])
    for pair, m in five["mdbs"].items():
        assert mdbs[pair]["raw"].tobytes() == m["raw"].tobytes() and (mdbs[pair]["position"] == m["position"]).all(), pair
        assert (mdbs[pair]["scaffold"] == m["scaffold"]).all()


def test_a_profile_fed_set_equals_a_batch_fed_set(five):
    _assert_same_set(five["by_profile"], five)
    assert len(five["table"]) > 0 and sum(len(m["raw"]) for m in five["mdbs"].values()) > 0
    assert any(r["scaffold"] == "sc9" and r["compared_bases_count"] > 4096 for r in five["table"])       # more than one tile is covered
    assert not any(r["scaffold"] in ("sc3", "sc7") and "s1" in (r["name1"], r["name2"]) for r in five["table"])
    assert {r["mm"] for r in five["table"]} == {0, 1, 2, 3}


def test_a_sample_in_several_profile_calls(ctx, five):
    """every sample in two add_profile calls that cut a shuffled scaffold list at different places, each in chunks of at most 1000
    coverage entries (sc7, sc8, sc9 go alone): the same bytes"""
    from instrain_amd import compare
    st = compare.SampleSet(ctx, NAMES, LENGTHS, min_cov=5)
    order = [[5, 2, 8, 0, 9, 7, 1, 4, 6, 3], [9, 8, 7, 6, 5, 4, 3, 2, 1, 0], [3, 0, 4, 8, 1, 7, 2, 6, 5, 9], [1, 8, 0, 9, 2, 3, 4, 5, 6, 7],
             [6, 4, 7, 3, 8, 5, 0, 1, 2, 9]]
    for k, s in enumerate(five["samples"]):
        cut = 2 + k
        for part in (order[k][cut:], order[k][:cut]):
            st.add_profile(s.name, s.covT(part), s.snv(part), mm_values=s.values, max_entries=1000)
    _assert_same_set(st, five)
    st.close()


def test_a_sample_half_by_batch_and_half_by_profile(ctx, five):
    from instrain_amd import compare
    st = compare.SampleSet(ctx, NAMES, LENGTHS, min_cov=5)
    for k, s in enumerate(five["samples"]):
        first, second = [9, 1, 3, 5, 7], [0, 2, 4, 6, 8]
        b, names, bounds = s.batch(ctx, five["codes"], scaffolds=first)
        if k % 2:                                               # the batch half first, or the profile half first
            st.add_batch(s.name, b, names, bounds, mm_values=s.values)
            st.add_profile(s.name, s.covT(second), s.snv(second), mm_values=s.values)
        else:
            st.add_profile(s.name, s.covT(second), s.snv(second), mm_values=s.values)
            st.add_batch(s.name, b, names, bounds, mm_values=s.values)
        b.close()
    _assert_same_set(st, five)
    st.close()


def test_determinism_and_strain_clusters(ctx, five):
    from instrain_amd import compare
    again = compare.SampleSet(ctx, NAMES, LENGTHS, min_cov=5)
    for s in five["samples"]:
        again.add_profile(s.name, s.covT(), s.snv(), mm_values=s.values)
    _assert_same_set(again, five)
    assert _levels_of(again) == _levels_of(five["by_profile"])
    again.close()
    stb = {n: "g1" for n in NAMES}
    five["by_batch"].compare(min_freq=0.05)
    five["by_profile"].compare(min_freq=0.05)
    a, b = five["by_batch"].strain_clusters(stb), five["by_profile"].strain_clusters(stb)
    pd.testing.assert_frame_equal(a, b)
    assert len(a) == 5 and five["by_batch"].cluster_pairs().tobytes() == five["by_profile"].cluster_pairs().tobytes()


# ---- 4. hand-built coverage edges against numpy ----
EDGE_LENGTHS = [1, 63, 64, 65, 4096, 4097, 8193]
EDGE_NAMES = ["e%d" % i for i in range(len(EDGE_LENGTHS))]
BIG = 2 ** 32 - 1


def _edge_covT():
    """levels 0, 1, 4, 9.  Every scaffold: 5 at its first and last position (level 0)."""
    c = {n: {0: {0: 5, ln - 1: 5}} for n, ln in zip(EDGE_NAMES, EDGE_LENGTHS)}
    e5, e6 = c["e5"], c["e6"]
    e5[0].update({100: 3, 101: 3, 200: BIG, 4095: 1})
    e5[1] = {100: 2, 101: 1}                                    # 100 reaches 5 only by cumulation, 101 stops at 4; level 1 is a key of e5 alone
    e5[4] = {200: BIG, 4095: 3, 4096: 1}                        # 2^32 - 1 at two levels: covered, no wrap; 4095 reaches 4, then ...
    e5[9] = {4095: 1, 4096: 3}                                  # ... 5 (the last position of the first tile; 4096 is the second tile)
    e6[0].update({4095: 5, 4096: 4, 8191: 2})                   # (8192, its last position, is the third tile)
    e6[4] = {10: 7, 4096: 1}                                    # the third tile (8192) has no entry at this level
    e6[9] = {8191: 3}
    c["e2"][9] = {}                                             # a present key with an empty series
    c["e4"][4] = {4095: 1, 0: 1}
    return {n: {mm: _ser(sorted(d), [d[p] for p in sorted(d)]) for mm, d in lv.items()} for n, lv in c.items()}


@pytest.mark.parametrize("min_cov", [5, 1])
def test_hand_built_edges_against_numpy(ctx, min_cov):
    from instrain_amd import compare
    covT = _edge_covT()
    full = {n: {0: _ser(np.arange(ln), np.full(ln, 7))} for n, ln in zip(EDGE_NAMES, EDGE_LENGTHS)}
    st = compare.SampleSet(ctx, EDGE_NAMES, EDGE_LENGTHS, min_cov=min_cov)
    st.add_profile("x", covT)                                   # (no SNV table at all)
    st.add_profile("full", full, pd.DataFrame())
    table = st.compare(min_freq=0.05)
    levels = st.levels
    st.close()
    axis = [0, 1, 4, 9]
    assert levels.shape == (1, len(EDGE_NAMES), len(axis))
    for sc, (n, ln) in enumerate(zip(EDGE_NAMES, EDGE_LENGTHS)):
        cum = np.zeros(ln, dtype=object)                        # Python integers: 2 x (2^32 - 1) is no trouble here
        for a, mm in enumerate(axis):
            if mm in covT[n]:
                for p, v in covT[n][mm].items():
                    cum[p] += int(v)
            r = levels[0, sc, a]
            both = int(sum(1 for v in cum if v >= min_cov))
            assert (int(r["both"]), int(r["either"]), int(r["mm"])) == (both, ln, mm), (n, mm)
            assert (int(r["present_a"]), int(r["present_b"])) == (int(mm in covT[n]), int(mm == 0)), (n, mm)
    rows = {(r["scaffold"], r["mm"]): r["compared_bases_count"] for r in table}
    assert sorted(mm for s, mm in rows if s == "e3") == [0] and sorted(mm for s, mm in rows if s == "e2") == [0, 9]
    assert sorted(mm for s, mm in rows if s == "e5") == [0, 1, 4, 9] and sorted(mm for s, mm in rows if s == "e6") == [0, 4, 9]
    if min_cov == 5:                                            # spelled out for e5: first, last, 200 | + 100 | 4095 is at 4 | + 4095
        assert [rows[("e5", mm)] for mm in axis] == [3, 4, 4, 5] and rows[("e2", 9)] == rows[("e2", 0)] == 2


# ---- 5. SNV rows ----
def _row(scaffold, position, mm, ref, con, var="A", allele_count=1, counts=None):
    cnt = dict(A=0, C=0, T=0, G=0)
    cnt.update(counts or {con: 20})
    return dict(scaffold=scaffold, position=position, position_coverage=sum(cnt.values()), allele_count=allele_count, ref_base=ref,
                con_base=con, var_base=var, mm=mm, **cnt)


def test_snv_rows_of_a_stored_table(ctx):
    from instrain_amd import compare
    names, lengths = ["p", "n", "q"], [100, 50, 70]
    cov = lambda ln, keys: {mm: _ser(np.arange(ln), np.full(ln, 9)) for mm in keys}
    a_cov = {"p": cov(100, (0, 2)), "n": cov(50, (0,))}         # `a` lacks q
    b_cov = {"p": cov(100, (0,)), "n": cov(50, (0,)), "q": cov(70, (0,))}
    a_rows = pd.DataFrame([
        _row("p", 10, 2, "A", "G"), _row("p", 10, 0, "A", "C"), _row("p", 10, 1, "A", "T"),     # one position, unsorted mm: the mm 2 row counts
        _row("p", 20, 0, "A", "A"), _row("p", 20, 1, "A", "C"),                                 # mm 1 is no level of `a`: still its last row
        _row("p", 30, 2, "C", "C"),                                                             # con == ref, the reference still seen: no SNP
        _row("n", 5, 0, "N", "A"),                                                              # reference N in one sample only: the scaffold fails
        _row("q", 3, 0, "A", "C"), _row("zzz", 3, 0, "A", "C")])                                # a scaffold `a` has no covT for; one the set lacks
    st = compare.SampleSet(ctx, names, lengths, min_cov=5)
    st.add_profile("a", a_cov, a_rows)
    st.add_profile("b", b_cov, None)
    logs = []
    table = st.compare(min_freq=0.05, logs=logs)
    m = st.mismatch_locations("a", "b")
    st.close()
    assert [(r["scaffold"], r["mm"], r["consensus_SNPs"], r["population_SNPs"], r["compared_bases_count"]) for r in table] == \
        [("p", 0, 2, 2, 100), ("p", 2, 2, 2, 100)]
    assert len(logs) == 1 and "DEBUG FAILURE CompareScaffold n ['a', 'b']" in logs[0]
    raw = m["raw"]
    assert m["scaffold"].tolist() == [0] * 4 and m["position"].tolist() == [10, 20, 10, 20] and raw["mm"].tolist() == [0, 0, 2, 2]
    assert raw["con_a"].tolist() == [3, 1, 3, 1] and raw["ref_a"].tolist() == [0] * 4 and raw["has_a"].tolist() == [1] * 4
    assert raw["has_b"].tolist() == [0] * 4 and raw["cnt_a"].tolist() == [[0, 0, 0, 20], [0, 20, 0, 0]] * 2
    assert raw["consensus_snp"].tolist() == [1] * 4 and raw["population_snp"].tolist() == [1] * 4


# ---- 6. refusals: the set stays as it was ----
def _raw_add(st, sample, ids, levels, present, off, pos, val, snv=None):
    ids, levels = np.ascontiguousarray(ids, dtype=np.int32), np.ascontiguousarray(levels, dtype=np.int32)
    present, off = np.ascontiguousarray(present, dtype=np.uint8), np.ascontiguousarray(off, dtype=np.int64)
    pos, val = np.ascontiguousarray(pos, dtype=np.uint32), np.ascontiguousarray(val, dtype=np.uint32)
    n_snv = 0 if snv is None else len(snv)
    return st.lib.isx_cmpset_add_profile(st.h, sample, len(ids), ids.ctypes.data, len(levels), levels.ctypes.data, present.ctypes.data,
                                         off.ctypes.data, pos.ctypes.data, val.ctypes.data, n_snv, None if snv is None else snv.ctypes.data, None)


def test_refusals_leave_the_set_as_it_was(ctx):
    from instrain_amd import _lib, compare
    names, lengths = ["p", "q", "r"], [100, 70, 4097]
    cov = lambda ln, keys, v=9: {mm: _ser(np.arange(0, ln, 2), np.full((ln + 1) // 2, v)) for mm in keys}
    st = compare.SampleSet(ctx, names, lengths, min_cov=5)
    st.add_profile("a", {"p": cov(100, (0, 2)), "r": cov(4097, (0,))}, pd.DataFrame([_row("p", 10, 2, "A", "G"), _row("r", 4096, 0, "A", "C")]))
    st.add_profile("b", {"p": cov(100, (0,)), "q": cov(70, (0,)), "r": cov(4097, (0, 1), 3)})
    before = _levels_of(st)
    mdb_before = st.mismatch_locations("a", "b")["raw"].tobytes()
    assert len(mdb_before) > 0

    def unchanged():
        assert _levels_of(st) == before and st.mismatch_locations("a", "b")["raw"].tobytes() == mdb_before and st.samples == ["a", "b"]

    with pytest.raises(_lib.IsxError) as e:                     # other level values than the sample's earlier call
        st.add_profile("a", {"q": cov(70, (0, 3))})
    assert e.value.code == -1
    unchanged()
    with pytest.raises(_lib.IsxError) as e:                     # the same scaffold twice
        st.add_profile("a", {"q": cov(70, (0, 2)), "p": cov(100, (0, 2))}, mm_values=[0, 2])
    assert e.value.code == -6
    unchanged()
    assert _raw_add(st, 0, [1, 0], [0, 2], [[1, 0], [1, 0]], [0, 1, 1, 2, 2], [5, 5], [9, 9]) == -6      # ... straight through the library
    assert _raw_add(st, 2, [1, 1], [0], [[1], [1]], [0, 1, 2], [5, 5], [9, 9]) == -6                       # ... and twice within one call
    unchanged()
    with pytest.raises(ValueError):                             # a profile of a longer scaffold than the set's
        st.add_profile("c", {"q": {0: _ser([0, 70], [9, 9])}})
    with pytest.raises(ValueError):
        st.add_profile("c", {"q": {0: _ser([0], [9])}}, pd.DataFrame([_row("q", 70, 0, "A", "C")]))
    unchanged()
    for pos in ([7, 6], [6, 6], [6, 70], [70, 71]):             # descending, duplicate, beyond the scaffold
        assert _raw_add(st, 2, [1], [0], [[1]], [0, 2], pos, [9, 9]) == -1
    assert _raw_add(st, 2, [1], [0, 1], [[1, 0]], [0, 1, 2], [6, 7], [9, 9]) == -1                         # an entry under a level that is no key
    assert _raw_add(st, 2, [1, 0], [0], [[1], [1]], [0, 2, 1], [6, 7], [9, 9]) == -1                       # offsets that descend
    assert _raw_add(st, 2, [3], [0], [[1]], [0, 1], [6], [9]) == -1                                        # a scaffold the set has not
    assert _raw_add(st, 2, [1], [2, 2], [[1, 1]], [0, 1, 2], [6, 7], [9, 9]) == -1                         # levels that do not ascend
    snv = np.zeros(1, dtype=_lib.PROFILE_SNV_DT)
    for field, bad in (("scaffold", 1), ("scaffold", -1), ("position", 70), ("mm", 65536), ("mm", -1), ("con_base", 4), ("var_base", 4), ("ref_base", 5)):
        row = snv.copy()
        row[field] = bad
        assert _raw_add(st, 2, [1], [0], [[1]], [0, 1], [6], [9], row) == -1, field
    unchanged()
    many = np.arange(129)                                       # 129 levels
    assert _raw_add(st, 2, [1], many, np.ones((1, 129)), np.r_[0, np.ones(129)], [6], [9]) == -3
    with pytest.raises(_lib.IsxError) as e:
        st.add_profile("c", {"q": {0: _ser([6], [9])}}, mm_values=many)
    assert e.value.code == -3
    unchanged()
    pooled = compare.SampleSet(ctx, names, lengths, min_cov=5, pooling=True)
    with pytest.raises(_lib.IsxError) as e:                     # a set with pooling takes resident batches only
        pooled.add_profile("a", {"p": cov(100, (0,))})
    assert e.value.code == -6 and pooled.samples == []
    assert _raw_add(pooled, 0, [0], [0], [[1]], [0, 1], [6], [9]) == -6
    pooled.close()
    # a call with no scaffold of the set does nothing, and says so
    assert _raw_add(st, 2, [-1], [0], [[1]], [0, 1], [6], [9]) == 0
    unchanged()
    st.add_profile("a", {"q": cov(70, (0, 2))})                 # and the set still takes what it should
    assert _levels_of(st) != before
    st.close()


# ---- 8. end to end: a BAM profiled live into a set, and the same profiles stored, loaded and added ----
def _have_hdf5():
    from instrain_amd.profile import emitters
    try:
        emitters._backend()
        return True
    except Exception:
        return False


@pytest.mark.skipif(not _have_hdf5(), reason="no h5py / libhdf5 on this host")
def test_profile_store_load_compare_equals_the_live_route(ctx, tmp_path):
    import instrain_amd.profile as prof
    from instrain_amd import compare
    from tests.test_oracle_golden import read_fasta
    lut, fb = util.load_lut()
    model = {int(i): int(v) for i, v in enumerate(lut) if v >= 0}
    model[-1] = fb
    seq = read_fasta(os.path.join(util.GOLD, "sars_cov_2_MT039887.1.fasta"))
    bam = os.path.join(util.GOLD, "sars_cov_2.sorted.bam")
    live = compare.SampleSet(ctx, ["MT039887.1"], [len(seq)], min_cov=5)
    stored = compare.SampleSet(ctx, ["MT039887.1"], [len(seq)], min_cov=5)
    for name, ani in (("ani95", 0.95), ("ani99", 0.99)):
        splits = prof.profile_bam(bam, s2s={"MT039887.1": seq}, null_model=model, min_cov=5, min_freq=0.05, min_snp=20, min_read_ani=ani,
                                  ctx=ctx, compare_set=live, compare_sample=name, strict=True)
        folder = str(tmp_path / name / "raw_data")
        compare.store_sample(folder, splits)
        stored.add_profile(name, *compare.load_sample(folder))
    t_live, t_stored = live.compare(min_freq=0.05), stored.compare(min_freq=0.05)
    _same_rows(t_stored, t_live)
    assert len(t_live) > 1 and t_live[-1]["compared_bases_count"] > 0
    a, b = live.mismatch_locations("ani95", "ani99"), stored.mismatch_locations("ani95", "ani99")
    assert _mdb_rows(a) == _mdb_rows(b)
    live.close()
    stored.close()
