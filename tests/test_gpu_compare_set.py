"""GPU: a whole sample set compared from per-sample sketches (instrain_amd/compare.py SampleSet, isx_cmpset_*) against the reference's
golden vectors, the pinned two-batch path (compare.compare_scaffolds), oracle/compare.py and plain numpy.  Everything compared is an
integer or a float made by the identical host expression: equality throughout."""
import itertools
import re

import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu

LENGTHS = [1, 63, 64, 65, 127, 128, 129, 4096, 4097]         # word edges, a scaffold inside one word, a tile edge (4096 = 64 words)
NAMES = ["sc%d" % i for i in range(len(LENGTHS))]
SB = np.r_[0, np.cumsum(LENGTHS)]
RAW_FIELDS = ("mm", "consensus_snp", "population_snp", "has_a", "has_b", "con_a", "ref_a", "var_a", "con_b", "ref_b", "var_b")


@pytest.fixture(scope="module")
def ctx():
    from instrain_amd import engine
    c = engine.Context(0)
    lut, fb = util.load_lut()
    c.set_null_model(lut, fb)
    yield c
    c.close()


def _batch(ctx, codes, bounds, pos, base, mm, n_mm):
    from instrain_amd import engine
    b = engine.Batch(ctx, codes, bounds, engine.pack_obs(pos.astype(np.uint32), base, mm), np.arange(len(pos), dtype=np.uint32),
                     n_mm_bins=n_mm, enable_linkage=False)
    b.run()
    return b


def _same_rows(got, exp):
    """two comparisonsTable row lists: every field equal, NaN == NaN"""
    assert len(got) == len(exp), (len(got), len(exp))
    for g, e in zip(got, exp):
        assert g.keys() == e.keys()
        for k in e:
            assert g[k] == e[k] or (g[k] != g[k] and e[k] != e[k]), (k, g, e)


def _mdb_rows(mdb):
    raw = mdb["raw"]
    return sorted(zip(mdb["scaffold"].tolist(), mdb["position"].tolist(), *(raw[f].tolist() for f in RAW_FIELDS),
                      map(tuple, raw["cnt_a"].tolist()), map(tuple, raw["cnt_b"].tolist())))


# ---- 1. the reference's vectors through the set ----
@pytest.mark.parametrize("name", ["compare_a", "compare_b", "compare_c", "compare_d"])
def test_reference_vectors_through_the_set(ctx, name):
    from instrain_amd import compare, engine
    g = util.load_case(name)
    codes = engine.encode_seq(str(g["seq"]))
    st = compare.SampleSet(ctx, ["scaffold"], [len(codes)], min_cov=5)
    for s in "ab":
        b = _batch(ctx, codes, [0, len(codes)], g[s + "_pos"], g[s + "_base"], g[s + "_mm"], int(g[s + "_mm"].max()) + 1)
        st.add_batch(s, b, ["scaffold"], [0, len(codes)])
        b.close()
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
    assert st.device_ms > 0


# ---- 2. / 3. five samples, every pair against the pinned pair path and the oracle ----
class Sample:
    """observations over the LENGTHS space; `mm` are device levels, `values` their real mm (None: level k is mm k)"""

    def __init__(self, name, seed, depth, n_levels, values=None, drop=()):
        from tests.test_gpu_parity import _random_split
        self.name, self.values, self.n_levels = name, values, n_levels
        _, pos, base, mm, _ = _random_split(seed, int(SB[-1]), depth, n_levels, 60)
        keep = np.ones(len(pos), bool)
        for sc in drop:                                          # no coverage at all on these scaffolds
            keep &= ~((pos >= SB[sc]) & (pos < SB[sc + 1]))
        self.pos, self.base = pos[keep], base[keep]
        self.mm = (mm[keep] if n_levels > 1 else mm[keep] * 0).astype(np.int64)
        self.real_mm = self.mm if values is None else np.asarray(values)[self.mm]
        self.has = [bool(((self.pos >= SB[sc]) & (self.pos < SB[sc + 1]) & (self.base < 4)).any()) for sc in range(len(LENGTHS))]

    def arrays(self, codes, scaffolds=None, real=False):
        """the observations on the given scaffolds, in the given order (None: all, set order), as a flat space of their own;
        real: levels = real mm -> (reference codes, bounds, pos, base, mm, n_mm, scaffold names)"""
        scaffolds = list(range(len(LENGTHS))) if scaffolds is None else list(scaffolds)
        bounds = np.r_[0, np.cumsum([LENGTHS[sc] for sc in scaffolds])]
        sel, new_pos = [], []
        for k, sc in enumerate(scaffolds):
            idx = np.flatnonzero((self.pos >= SB[sc]) & (self.pos < SB[sc + 1]))
            sel.append(idx)
            new_pos.append(self.pos[idx] - SB[sc] + bounds[k])
        sel, new_pos = np.concatenate(sel), np.concatenate(new_pos)
        mm = self.real_mm if real else self.mm
        n_mm = int(np.max(self.values)) + 1 if (real and self.values is not None) else self.n_levels
        ref = np.concatenate([codes[SB[sc]:SB[sc + 1]] for sc in scaffolds])
        return ref, bounds, new_pos, self.base[sel], mm[sel], n_mm, [NAMES[sc] for sc in scaffolds]

    def batch(self, ctx, codes, scaffolds=None, real=False):
        """-> (a run batch of those observations, its scaffold names, its bounds)"""
        ref, bounds, pos, base, mm, n_mm, names = self.arrays(codes, scaffolds, real)
        return _batch(ctx, ref, bounds, pos, base, mm, n_mm), names, bounds


@pytest.fixture(scope="module")
def five(ctx):
    """the five samples, the pinned pair path's answer for each of the 10 pairs, and the set's"""
    from instrain_amd import compare, engine
    from tests.test_gpu_parity import _random_split
    seq = re.sub("[^ACGT]", "A", _random_split(700, int(SB[-1]), 5, 1, 10)[0])        # a reference without N
    codes = engine.encode_seq(seq)
    samples = [Sample("s0", 701, 30, 1), Sample("s1", 702, 24, 1, drop=(3, 7)), Sample("s2", 703, 26, 4),
               Sample("s3", 704, 28, 3, values=[0, 1, 3]), Sample("s4", 705, 22, 2, values=[0, 2])]
    # the set: device levels + level_mm_values
    st = compare.SampleSet(ctx, NAMES, LENGTHS, min_cov=5)
    for s in samples:
        b, names, bounds = s.batch(ctx, codes)
        st.add_batch(s.name, b, names, bounds, mm_values=s.values)
        b.close()
    table = st.compare(min_freq=0.05)
    levels = st.levels.copy()
    mdbs = {(a.name, b.name): st.mismatch_locations(a.name, b.name) for a, b in itertools.combinations(samples, 2)}
    st.close()
    # the pinned pair path on resident batches whose levels ARE the real mm (what level_mm_values stands for), so its level k is mm k
    pinned = {}
    resident = [s.batch(ctx, codes, real=True)[0] for s in samples]
    for (i, a), (j, b) in itertools.combinations(enumerate(samples), 2):
        t, m, _ = compare.compare_scaffolds(resident[i], resident[j], SB, NAMES, a.name, b.name, min_cov=5, min_freq=0.05,
                                            store_mismatch_locations=True)
        pinned[(a.name, b.name)] = (t, m)
    for b in resident:
        b.close()
    return dict(seq=seq, codes=codes, samples=samples, table=table, levels=levels, mdbs=mdbs, pinned=pinned)


def _expected_from_pinned(five):
    """the pinned pair tables in the set's order, without the scaffolds either sample lacks; the Mdb rows at the levels the pair's
    table has on that scaffold (the reference makes rows only at the union of the two covTs' keys)"""
    samples, exp_table, exp_mdb, dropped = five["samples"], [], {}, 0
    for sc, name in enumerate(NAMES):
        for a, b in itertools.combinations(samples, 2):
            t, _ = five["pinned"][(a.name, b.name)]
            assert not any(r.get("failed") for r in t)
            rows = [r for r in t if r["scaffold"] == name]
            if not (a.has[sc] and b.has[sc]):
                dropped += 1 if rows else 0
                continue
            exp_table += rows
    for a, b in itertools.combinations(samples, 2):
        t, m = five["pinned"][(a.name, b.name)]
        levels_of = {(NAMES.index(r["scaffold"]), r["mm"]) for r in t}
        exp_mdb[(a.name, b.name)] = [r for r in _mdb_rows(m) if a.has[r[0]] and b.has[r[0]] and (r[0], r[2]) in levels_of]
    return exp_table, exp_mdb, dropped


def test_every_pair_equals_the_pinned_pair_path(five):
    exp_table, exp_mdb, dropped = _expected_from_pinned(five)
    _same_rows(five["table"], exp_table)
    for pair, rows in exp_mdb.items():
        assert _mdb_rows(five["mdbs"][pair]) == rows, pair
    assert sum(len(r) for r in exp_mdb.values()) > 0 and dropped > 0               # not vacuous: SNP rows exist, a (pair, scaffold) is dropped
    assert not any(r["scaffold"] in ("sc3", "sc7") and "s1" in (r["name1"], r["name2"]) for r in five["table"])
    assert {r["mm"] for r in five["table"]} == {0, 1, 2, 3}                           # the union of the samples' real mm values


def test_every_pair_equals_the_oracle(five):
    """the same set against oracle/compare.py, scaffold by scaffold: not against product code alone"""
    from oracle import compare as ocompare, oracle
    lut, fb = util.load_lut()
    samples, seq = five["samples"], five["seq"]
    prof = {}
    for s in samples:
        for sc in range(len(LENGTHS)):
            k = (s.pos >= SB[sc]) & (s.pos < SB[sc + 1])
            prof[(s.name, sc)] = oracle.profile_split(s.pos[k] - SB[sc], s.base[k], s.real_mm[k], np.arange(int(k.sum())),
                                                      seq[SB[sc]:SB[sc + 1]], 0, lut, fb)
    exp_table, exp_rows = [], {}
    for sc in range(len(LENGTHS)):
        for a, b in itertools.combinations(samples, 2):
            if not (a.has[sc] and b.has[sc]):
                continue
            ra, rb = prof[(a.name, sc)], prof[(b.name, sc)]
            o, c = ocompare.calc_mm2overlap(ra["entries"], rb["entries"], LENGTHS[sc], min_cov=5)
            rows = ocompare.compare_snp_tables(ra["snv"], rb["snv"], o, lut, fb, min_freq=0.05)
            exp_rows.setdefault((a.name, b.name), []).extend((sc, mm, p, cc, q) for mm, p, cc, q in rows)
            for t in ocompare.overlap_table(o, c, rows, LENGTHS[sc]):
                exp_table.append((NAMES[sc], a.name, b.name, t["mm"], t["compared_bases_count"], t["consensus_SNPs"], t["population_SNPs"],
                                  t["coverage_overlap"]))
    got = [(r["scaffold"], r["name1"], r["name2"], r["mm"], r["compared_bases_count"], r["consensus_SNPs"], r["population_SNPs"],
            r["coverage_overlap"]) for r in five["table"]]
    assert got == exp_table
    n_rows = 0
    for a, b in itertools.combinations(samples, 2):
        m = five["mdbs"][(a.name, b.name)]
        got_rows = sorted(zip(m["scaffold"].tolist(), m["raw"]["mm"].tolist(), m["position"].tolist(),
                              m["raw"]["consensus_snp"].astype(bool).tolist(), m["raw"]["population_snp"].astype(bool).tolist()))
        assert got_rows == sorted(exp_rows.get((a.name, b.name), [])), (a.name, b.name)
        n_rows += len(got_rows)
    assert n_rows > 0


def test_a_sample_in_pieces(ctx, five):
    """every sample through two batches that cut the scaffold list at different places, in another scaffold order, each closed before
    compare(): the same bytes as from whole batches -- the sketch does not lean on the batch"""
    from instrain_amd import compare
    st = compare.SampleSet(ctx, NAMES, LENGTHS, min_cov=5)
    order = [[5, 2, 8, 0, 7, 1, 4, 6, 3], [8, 7, 6, 5, 4, 3, 2, 1, 0], [3, 0, 4, 8, 1, 7, 2, 6, 5], [1, 8, 0, 2, 3, 4, 5, 6, 7],
             [6, 4, 7, 3, 8, 5, 0, 1, 2]]
    for k, s in enumerate(five["samples"]):
        cut = 2 + k
        for part in (order[k][cut:], order[k][:cut]):
            b, names, bounds = s.batch(ctx, five["codes"], scaffolds=part)
            st.add_batch(s.name, b, names, bounds, mm_values=s.values)
            b.close()
    table = st.compare(min_freq=0.05)
    assert st.levels.tobytes() == five["levels"].tobytes()
    _same_rows(table, five["table"])
    for pair, m in five["mdbs"].items():
        got = st.mismatch_locations(*pair)
        assert got["raw"].tobytes() == m["raw"].tobytes() and (got["position"] == m["position"]).all()
    st.close()


def test_pipe_slots_feed_the_set(ctx, five):
    """samples through pipe slots instead of run batches: a one-level pipe whose single slot two samples use in turn (the shrunk
    dense hand-back, no count table) and a 4-level pipe (the level-sparse hand-back); every slot is released before compare()"""
    from instrain_amd import compare, engine
    samples = five["samples"][:3]
    st = compare.SampleSet(ctx, NAMES, LENGTHS, min_cov=5)
    pipes = {}
    for s in samples:
        ref, bounds, pos, base, mm, n_mm, names = s.arrays(five["codes"])
        if n_mm not in pipes:
            pipes[n_mm] = engine.Pipe(ctx, max_pos=int(SB[-1]), max_obs=max(len(x.pos) for x in samples), max_splits=16, depth=1,
                                      host_threads=2, n_mm_bins=n_mm)
        t = pipes[n_mm].submit(ref, bounds, engine.pack_obs(pos.astype(np.uint32), base, mm), np.arange(len(pos), dtype=np.uint32))
        res = pipes[n_mm].collect(t)
        st.add_batch(s.name, res["slot"], names, bounds, mm_values=s.values)
        pipes[n_mm].release(t)
    for p in pipes.values():
        p.close()
    table = st.compare(min_freq=0.05)
    exp = [r for r in five["table"] if {r["name1"], r["name2"]} <= {"s0", "s1", "s2"}]
    _same_rows(table, exp)
    for pair in (("s0", "s1"), ("s0", "s2"), ("s1", "s2")):
        got, m = st.mismatch_locations(*pair), five["mdbs"][pair]
        assert got["raw"].tobytes() == m["raw"].tobytes()
    st.close()
    assert len(pipes) == 2 and len(exp) > 0


def test_scaffolds_the_set_does_not_name_are_skipped(ctx, five):
    """a set of three of the nine scaffolds, in another order than the batches': the other six are left out (set_scaffold_ids -1)"""
    from instrain_amd import compare
    mine = ["sc8", "sc2", "sc6"]
    st = compare.SampleSet(ctx, mine, [LENGTHS[NAMES.index(n)] for n in mine], min_cov=5)
    for s in five["samples"][:3]:
        b, names, bounds = s.batch(ctx, five["codes"])
        st.add_batch(s.name, b, names, bounds, mm_values=s.values)
        b.close()
    table = st.compare(min_freq=0.05)
    st.close()
    exp = [r for n in mine for r in five["table"] if r["scaffold"] == n and {r["name1"], r["name2"]} <= {"s0", "s1", "s2"}]
    _same_rows(table, exp)
    assert len(exp) > 0


# ---- 4. more than one wave of pairs, more than one block of samples ----
@pytest.mark.parametrize("n_samples,lengths", [(12, [65, 1, 200]), (70, [65, 1, 3100])])
def test_many_tiny_samples_vs_numpy(ctx, n_samples, lengths):
    """66 pairs: more than one wave of them; 70 samples: two sample blocks (the staged tile then holds fewer words: the 3100-position
    scaffold is more than one tile)"""
    from instrain_amd import compare, engine
    sb = np.r_[0, np.cumsum(lengths)]
    rng = np.random.Generator(np.random.PCG64(4100 + n_samples))
    codes = engine.encode_seq("".join("ACGT"[i] for i in rng.integers(0, 4, size=int(sb[-1]))))
    st = compare.SampleSet(ctx, ["x", "y", "z"], lengths, min_cov=5)
    cov = []
    for k in range(n_samples):
        pos = rng.integers(0, sb[-1], size=int(sb[-1]) * 7)
        if k % 5 == 3:
            pos = pos[pos != sb[1]]                              # no read on the one-position scaffold
        base = rng.integers(0, 4, size=len(pos)).astype(np.uint8)
        b = _batch(ctx, codes, sb, pos, base, np.zeros(len(pos), np.int64), 1)
        st.add_batch("t%d" % k, b, ["x", "y", "z"], sb)
        b.close()
        cov.append(np.bincount(pos, minlength=int(sb[-1])))
    st.compare()
    levels = st.levels
    st.close()
    pairs = list(itertools.combinations(range(n_samples), 2))
    assert levels.shape == (len(pairs), 3, 1) and len(pairs) > 64
    absent = 0
    for p, (i, j) in enumerate(pairs):
        for sc in range(3):
            r = levels[p, sc, 0]
            c1, c2 = cov[i][sb[sc]:sb[sc + 1]], cov[j][sb[sc]:sb[sc + 1]]
            if not (c1.any() and c2.any()):
                assert r["present_a"] == 0 and r["present_b"] == 0
                absent += 1
                continue
            t1, t2 = c1 >= 5, c2 >= 5
            assert (r["both"], r["either"], r["mm"]) == (int((t1 & t2).sum()), int((t1 | t2).sum()), 0), (i, j, sc)
            assert r["present_a"] == 1 and r["present_b"] == 1 and r["consensus_snps"] >= 0
    assert absent > 0


# ---- 5. the failure rule ----
def test_a_failing_pair_takes_the_whole_scaffold(ctx):
    from instrain_amd import compare, engine
    lengths, depth = [300, 200], 12
    sb = np.r_[0, np.cumsum(lengths)]
    rng = np.random.Generator(np.random.PCG64(55))
    ref = rng.integers(0, 4, size=int(sb[-1])).astype(np.uint8)              # codes 0..3 = A C T G
    seq = "".join("ACTG"[c] for c in ref)
    seq = seq[:100] + "N" + seq[101:]
    codes = engine.encode_seq(seq)

    def sample(n_at, snp_at_350):
        """every position `depth` reads deep showing the reference; position 100 (reference N): 'A' x depth or no read at all;
        position 350 (scaffold 1, position 50): a consensus SNP or the reference"""
        pos = np.repeat(np.arange(int(sb[-1])), depth)
        base = ref[pos].copy()
        base[pos == 100] = 0
        if snp_at_350:
            base[pos == 350] = (ref[350] + 1) % 4
        k = np.ones(len(pos), bool) if n_at else pos != 100
        return pos[k], base[k]
    obs = {"A": sample(True, True), "B": sample(False, False), "C": sample(True, False)}
    batches = {n: _batch(ctx, codes, sb, p, b, np.zeros(len(p), np.int64), 1) for n, (p, b) in obs.items()}
    # what the pinned pair path says of each pair alone
    alone = {pair: compare.compare_scaffolds(batches[pair[0]], batches[pair[1]], sb, ["n", "ok"])[0] for pair in (("A", "B"), ("A", "C"), ("B", "C"))}
    assert alone[("A", "B")][0] == {"scaffold": "n", "failed": True} and alone[("B", "C")][0] == {"scaffold": "n", "failed": True}
    assert not any(r.get("failed") for r in alone[("A", "C")]) and alone[("A", "C")][0]["scaffold"] == "n"      # alone, this pair passes
    st = compare.SampleSet(ctx, ["n", "ok"], lengths, min_cov=5)
    for n in "ABC":
        st.add_batch(n, batches[n], ["n", "ok"], sb)
        batches[n].close()
    logs = []
    table = st.compare(min_freq=0.05, logs=logs)
    assert [r["scaffold"] for r in table] == ["ok"] * 3 and [(r["name1"], r["name2"]) for r in table] == [("A", "B"), ("A", "C"), ("B", "C")]
    assert [r["consensus_SNPs"] for r in table] == [1, 1, 0] and all(r["compared_bases_count"] == 200 for r in table)
    assert len(logs) == 1 and "DEBUG FAILURE CompareScaffold n ['A', 'B', 'C']" in logs[0]
    for pair in alone:
        m = st.mismatch_locations(*pair)
        assert (m["scaffold"] == 1).all()
    assert len(st.mismatch_locations("A", "B")["raw"]) == 1 and st.mismatch_locations("A", "B")["position"].tolist() == [50]
    st.close()


# ---- 6. determinism and argument errors ----
def test_determinism_and_argument_errors(ctx, five):
    from instrain_amd import compare, engine
    from instrain_amd._lib import IsxError
    samples, codes = five["samples"], five["codes"]
    st = compare.SampleSet(ctx, NAMES, LENGTHS, min_cov=5)
    for s in samples[:4]:
        b, names, bounds = s.batch(ctx, codes)
        st.add_batch(s.name, b, names, bounds, mm_values=s.values)
        b.close()
    t1, l1 = st.compare(), st.levels.copy()
    t2, l2 = st.compare(), st.levels.copy()
    assert l1.tobytes() == l2.tobytes() and len(t1) == len(t2) > 0
    _same_rows(t1, t2)
    m1, m2 = st.mismatch_locations("s0", "s2"), st.mismatch_locations("s0", "s2")
    assert m1["raw"].tobytes() == m2["raw"].tobytes() and len(m1["raw"]) > 0
    # every refusal below is made on the host, before anything is launched
    b, names, bounds = samples[0].batch(ctx, codes, scaffolds=[4, 2])
    with pytest.raises(IsxError) as e:                           # (sample, scaffold) twice
        st.add_batch("s0", b, names, bounds)
    assert e.value.code == -6
    with pytest.raises(IsxError):                                # bounds that do not span the batch
        st.add_batch("fresh", b, names, bounds - np.r_[0, 0, 1])
    with pytest.raises(IsxError):                                # ... or do not ascend
        st.add_batch("fresh", b, names, np.r_[0, bounds[2], bounds[2]])
    with pytest.raises(IsxError):                                # a scaffold of another length than the set's
        st.add_batch("fresh", b, ["sc4", "sc3"], bounds)
    with pytest.raises(IsxError):                                # other level values than the sample's earlier batches
        st.add_batch("s3", b, ["nowhere", "sc2"], bounds, mm_values=[5])
    other = engine.Context(0)
    lut, fb = util.load_lut()
    other.set_null_model(lut, fb)
    st2 = compare.SampleSet(other, NAMES, LENGTHS, min_cov=5)
    with pytest.raises(IsxError):                                # a batch from another ctx
        st2.add_batch("s0", b, names, bounds)
    st2.close()
    other.close()
    b.close()
    assert st.compare() is not None and st.levels.tobytes() == l1.tobytes()            # the refused calls left the set as it was
    st.close()
