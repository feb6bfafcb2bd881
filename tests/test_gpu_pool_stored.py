"""GPU: SNV pooling from stored profiles and observations of their BAMs (compare.SampleSet.add_profile_pooled / pool_plan / pool_add_obs /
pool_obs_done: isx_cmpset_add_profile_pool, isx_cmpset_pool_add_obs, isx_cmpset_pool_obs_done) against the reference's own DSTdb / PMdb
from the reference's own stored tables (tests/golden/make_pool_stored_golden.py), against the live route (add_batch + pool_add) byte
for byte, against tests/pool_ref.py and, for k_pull_obs alone, against numpy's bincount.  Integers and strings only: equality."""
import os
import re

import numpy as np
import pandas as pd
import pytest

from tests import pool_ref, stored_ref, util

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LENGTHS = [1, 63, 64, 65, 127, 128, 129, 4096, 4097]
NAMES = ["sc%d" % i for i in range(len(LENGTHS))]
SB = np.r_[0, np.cumsum(LENGTHS)]
CLASSES = np.array(["AmbiguousReference", "DivergentSite", "SNS", "SNV", "con_SNV", "pop_SNV"], dtype=object)
ERR_ARG, ERR_STATE = -1, -6


@pytest.fixture(scope="module")
def ctx():
    from instrain_amd import engine
    c = engine.Context(0)
    lut, fb = util.load_lut()
    c.set_null_model(lut, fb)
    yield c
    c.close()


def _obs(pos, base, mm=None):
    from instrain_amd import engine
    pos = np.asarray(pos)
    return engine.pack_obs(pos.astype(np.uint32), np.asarray(base).astype(np.uint8), np.zeros(len(pos), np.int64) if mm is None else np.asarray(mm))


class Sample:
    """observations over a flat space of scaffolds laid end to end (bounds `sb`); `mm` are device levels, `values` their real mm"""

    def __init__(self, name, pos, base, mm, n_levels, values=None, sb=SB, names=NAMES):
        self.name, self.values, self.n_levels, self.sb, self.names = name, values, n_levels, np.asarray(sb), list(names)
        self.pos, self.base, self.mm = np.asarray(pos, np.int64), np.asarray(base, np.uint8), np.asarray(mm, np.int64)
        self.real_mm = self.mm if values is None else np.asarray(values)[self.mm]

    @classmethod
    def random(cls, name, seed, depth, n_levels, values=None, drop=()):
        from tests.test_gpu_parity import _random_split
        _, pos, base, mm, _ = _random_split(seed, int(SB[-1]), depth, n_levels, 60)
        keep = np.ones(len(pos), bool)
        for sc in drop:
            keep &= ~((pos >= SB[sc]) & (pos < SB[sc + 1]))
        return cls(name, pos[keep], base[keep], mm[keep] if n_levels > 1 else mm[keep] * 0, n_levels, values)

    def batch(self, ctx, codes, scaffolds=None):
        """-> (a run batch of the observations on the given scaffolds laid end to end in that order, their names, the bounds)"""
        from instrain_amd import engine
        lengths = np.diff(self.sb)
        scaffolds = list(range(len(lengths))) if scaffolds is None else list(scaffolds)
        bounds = np.r_[0, np.cumsum([lengths[sc] for sc in scaffolds])]
        sel, new_pos = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
        for k, sc in enumerate(scaffolds):
            idx = np.flatnonzero((self.pos >= self.sb[sc]) & (self.pos < self.sb[sc + 1]))
            sel.append(idx)
            new_pos.append(self.pos[idx] - self.sb[sc] + bounds[k])
        sel, new_pos = np.concatenate(sel), np.concatenate(new_pos)
        ref = np.concatenate([codes[self.sb[sc]:self.sb[sc + 1]] for sc in scaffolds])
        b = engine.Batch(ctx, ref, bounds, _obs(new_pos, self.base[sel], self.mm[sel]), np.arange(len(sel), dtype=np.uint32),
                         n_mm_bins=self.n_levels, enable_linkage=False)
        b.run()
        return b, [self.names[sc] for sc in scaffolds], bounds

    def stored(self, ctx, codes, scaffolds=None):
        """what a stored profile of the sample holds: (covT, the cumulative_snv_table with class / cryptic), the table fetched from a batch"""
        b, names, bounds = self.batch(ctx, codes, scaffolds)
        rows = b.fetch()["snv"]
        b.close()
        table = stored_ref.snv_frame(rows, bounds, names, mm_values=self.values)
        if len(rows):
            table["class"], table["cryptic"] = CLASSES[rows["cls"]], rows["cryptic"].astype(bool)
        keep = np.ones(len(self.names), bool) if scaffolds is None else np.isin(np.arange(len(self.names)), list(scaffolds))
        covT = stored_ref.covT_from_obs(self.pos, self.base, self.real_mm, self.sb, self.names)
        return {n: d for n, d in covT.items() if keep[self.names.index(n)]}, table

    def regions(self, plan):
        """the observations in the planned columns, one region per planned scaffold -> (names, obs with positions on the scaffold, offsets)"""
        names, parts, off = [], [], [0]
        for n, (lo, hi, _) in plan.items():
            sc = self.names.index(n)
            k = (self.pos >= self.sb[sc] + lo) & (self.pos < self.sb[sc] + hi)
            names.append(n)
            parts.append(_obs(self.pos[k] - self.sb[sc], self.base[k], self.mm[k]))
            off.append(off[-1] + int(k.sum()))
        return names, np.concatenate(parts) if parts else _obs([], []), off

    def observations(self):
        return (self.name, self.pos, self.base, self.real_mm)


def _pull_obs(st, s, only=None):
    plan = {n: w for n, w in st.pool_plan(s.name).items() if only is None or n in only}
    names, obs, off = s.regions(plan)
    st.pool_add_obs(s.name, names, obs, off)
    st.pool_obs_done(s.name, names)
    return plan


def _raw(st):
    dst, pm = st.pooled_tables()
    return dst, pm, b"".join(st.pool_raw[k].tobytes() for k in ("summary", "counts", "meta")) + st.pool_site_positions().tobytes()


# ---- 1. the reference's tables from the reference's stored tables ----
def _golden_stored(sample):
    z = np.load(os.path.join(GOLDEN, "pool_stored_%s_covT.npz" % sample))
    off, covT = z["series_offsets"], {}
    for k, (sc, mm) in enumerate(zip(z["series_scaffold"].tolist(), z["series_mm"].tolist())):
        covT.setdefault(str(sc), {})[int(mm)] = (z["positions"][off[k]:off[k + 1]], z["values"][off[k]:off[k + 1]])
    return covT, pd.read_csv(os.path.join(GOLDEN, "pool_stored_%s_snv.csv" % sample), keep_default_na=False)


def test_golden_stored_tables_through_the_device(ctx):
    from instrain_amd import compare
    g = np.load(os.path.join(GOLDEN, "pool_obs.npz"))
    names, lengths = [str(n) for n in g["names"]], g["lengths"].tolist()
    sb = np.r_[0, np.cumsum(lengths)]
    samples = [Sample(str(s), g[str(s) + "_pos"], g[str(s) + "_base"], g[str(s) + "_mm"], int(g[str(s) + "_mm"].max()) + 1, sb=sb, names=names)
               for s in g["samples"]]
    st = compare.SampleSet(ctx, names, lengths, min_cov=5, pooling=True)
    n_cryptic = 0
    for s in samples:
        covT, table = _golden_stored(s.name)
        n_cryptic += int(table["cryptic"].sum())
        st.add_profile_pooled(s.name, covT, table)
    assert n_cryptic > 0 and st.pool_sites() > 0
    plans = [_pull_obs(st, s) for s in samples]
    assert any(plans) and all(hi > lo and n > 0 for p in plans for lo, hi, n in p.values())
    dst, pm, _ = _raw(st)
    st.close()
    exp_dst, exp_pm = pool_ref.load_golden(GOLDEN, names)
    pool_ref.same_frames(dst, exp_dst)
    pool_ref.same_frames(pm, exp_pm)


# ---- 2. stored against live, byte for byte ----
@pytest.fixture(scope="module")
def five(ctx):
    from instrain_amd import compare, engine
    from tests.test_gpu_parity import _random_split
    seq = re.sub("[^ACGT]", "A", _random_split(700, int(SB[-1]), 5, 1, 10)[0])
    codes = engine.encode_seq(seq)
    samples = [Sample.random("s0", 701, 30, 1), Sample.random("s1", 702, 24, 1, drop=(3, 7)), Sample.random("s2", 703, 26, 4),
               Sample.random("s3", 704, 28, 3, values=[0, 1, 3]), Sample.random("s4", 705, 22, 2, values=[0, 2])]
    live = compare.SampleSet(ctx, NAMES, LENGTHS, min_cov=5, pooling=True)
    batches = [s.batch(ctx, codes) for s in samples]
    for s, (b, bn, bb) in zip(samples, batches):
        live.add_batch(s.name, b, bn, bb, mm_values=s.values)
    live.pool_sites()
    for s, (b, bn, bb) in zip(samples, batches):
        live.pool_add(s.name, b, bn, bb)
        b.close()
    dst, pm, raw = _raw(live)
    rows = live.compare()
    out = dict(seq=seq, codes=codes, samples=samples, dst=dst, pm=pm, raw=raw, rows=rows, levels=live.levels.tobytes(),
               stored={s.name: s.stored(ctx, codes) for s in samples})
    live.close()
    return out


def _same_as_live(st, five):
    dst, pm, raw = _raw(st)
    assert raw == five["raw"] and len(raw) > 0
    pool_ref.same_frames(dst, five["dst"])
    pool_ref.same_frames(pm, five["pm"])
    rows = st.compare()
    assert st.levels.tobytes() == five["levels"] and str(rows) == str(five["rows"]) and len(rows) > 0


def test_stored_equals_live(ctx, five):
    from instrain_amd import compare
    st = compare.SampleSet(ctx, NAMES, LENGTHS, min_cov=5, pooling=True)
    for s in five["samples"]:
        st.add_profile_pooled(s.name, *five["stored"][s.name], mm_values=s.values, max_entries=3000)
    assert st.pool_sites() > 50
    for s in five["samples"]:
        assert _pull_obs(st, s)
    _same_as_live(st, five)
    st.close()
    lut, fb = util.load_lut()
    exp_dst, exp_pm = pool_ref.pooled_tables([s.observations() for s in five["samples"]], five["seq"], NAMES, LENGTHS, lut, fb)
    pool_ref.same_frames(five["dst"], exp_dst)
    pool_ref.same_frames(five["pm"], exp_pm)


def test_one_sample_live_the_others_stored(ctx, five):
    from instrain_amd import compare
    st = compare.SampleSet(ctx, NAMES, LENGTHS, min_cov=5, pooling=True)
    s2 = five["samples"][2]
    b, bn, bb = s2.batch(ctx, five["codes"])
    for s in five["samples"]:
        if s is s2:
            st.add_batch(s.name, b, bn, bb, mm_values=s.values)
        else:
            st.add_profile_pooled(s.name, *five["stored"][s.name], mm_values=s.values)
    st.pool_sites()
    for s in five["samples"]:
        if s is s2:
            st.pool_add(s.name, b, bn, bb)
        else:
            _pull_obs(st, s)
    b.close()
    _same_as_live(st, five)
    st.close()


def test_every_sample_half_through_each_entry_point(ctx, five):
    """the odd scaffolds of every sample by batch (own rows and pull), the even ones from the stored profile and observations"""
    from instrain_amd import compare
    st = compare.SampleSet(ctx, NAMES, LENGTHS, min_cov=5, pooling=True)
    odd, even = [7, 1, 3, 5], [0, 2, 4, 6, 8]
    batches = []
    for k, s in enumerate(five["samples"]):
        covT, table = five["stored"][s.name]
        half = [NAMES[sc] for sc in even]
        covT, table = {n: d for n, d in covT.items() if n in half}, table[table["scaffold"].isin(half)] if len(table) else table
        batches.append(s.batch(ctx, five["codes"], odd))
        if k % 2:
            st.add_batch(s.name, *batches[-1], mm_values=s.values)
            st.add_profile_pooled(s.name, covT, table, mm_values=s.values)
        else:
            st.add_profile_pooled(s.name, covT, table, mm_values=s.values)
            st.add_batch(s.name, *batches[-1], mm_values=s.values)
    st.pool_sites()
    for s, (b, bn, bb) in zip(five["samples"], batches):
        _pull_obs(st, s, only=[NAMES[sc] for sc in even])
        st.pool_add(s.name, b, bn, bb)
        b.close()
    _same_as_live(st, five)
    st.close()


# ---- 3. k_pull_obs at its edges, against bincount ----
E_LENGTHS, E_NAMES = [1, 320, 2000], ["one", "edges", "deep"]
E_SB = np.r_[0, np.cumsum(E_LENGTHS)]
PLANTED = {0: [0], 1: [0, 63, 256, 319], 2: [100, 101, 1999]}


@pytest.fixture(scope="module")
def edges(ctx):
    """an all-A reference; X shows {A, C} at the planted sites (it owns them all) and A elsewhere, Y comes from a stored profile that
    covers everything and calls nothing: every site is Y's to pull"""
    from instrain_amd import compare, engine
    codes = engine.encode_seq("A" * int(E_SB[-1]))
    sites = np.concatenate([E_SB[sc] + np.array(p, np.int64) for sc, p in PLANTED.items()])
    covered = np.arange(E_SB[-1])
    is_site = np.isin(covered, sites)
    x_pos = np.concatenate([np.repeat(covered[~is_site], 6), np.repeat(covered[is_site], 20)])
    x_base = np.concatenate([np.zeros(6 * int((~is_site).sum()), np.uint8), np.tile(np.r_[np.zeros(10, np.uint8), np.ones(10, np.uint8)], len(sites))])
    X = Sample("X", x_pos, x_base, np.zeros(len(x_pos), np.int64), 1, sb=E_SB, names=E_NAMES)
    st = compare.SampleSet(ctx, E_NAMES, E_LENGTHS, min_cov=5, pooling=True)
    b, bn, bb = X.batch(ctx, codes)
    st.add_batch("X", b, bn, bb)
    b.close()
    st.add_profile_pooled("Y", {n: {0: (np.arange(ln), np.full(ln, 6))} for n, ln in zip(E_NAMES, E_LENGTHS)}, pd.DataFrame())
    assert st.pool_sites() == len(sites)
    assert st.pool_plan("Y") == {"one": (0, 1, 1), "edges": (0, 320, 4), "deep": (99, 2000, 3)} and st.pool_plan("X") == {}
    yield st
    st.close()


def _edge_regions():
    """-> (scaffold names, gpos0, [(positions, bases)] per region): hand-built observations of Y"""
    rng = np.random.Generator(np.random.PCG64(33))
    G0 = 1000                                                   # the regions of `edges` count their positions from 1000
    first = (np.r_[np.repeat([0, 1, 63], [5, 7, 9]), 63, 63], np.r_[rng.integers(0, 4, 21), 4, 4])          # a non-site (1); base 4 at a site
    second = (np.r_[np.repeat([64, 256, 319], [3, 4, 2])], rng.integers(0, 4, 9))                            # a non-site (64)
    # deep: 63 observations of a non-site, then a 1000-deep column at 100 (starts at lane 63 of wave 0), then fillers so that the
    # 1000-deep column at 1999 starts at the last lane of a 256-block, then sites 100 / 101 with alternating bases
    n_fill = (255 - (63 + 1000)) % 256
    pos = np.r_[np.full(63, 500), np.full(1000, 100), np.full(n_fill, 501), np.full(1000, 1999), np.tile([100, 101], 100)]
    base = np.r_[np.zeros(63, int), rng.integers(0, 4, 1000), np.zeros(n_fill, int), rng.integers(0, 5, 1000), np.tile([0, 1, 1, 0], 50)]
    assert (63 + 1000 + n_fill) % 256 == 255
    empty = (np.zeros(0, int), np.zeros(0, int))
    # the deep region comes FIRST: every call that holds it starts with it, so the alignments above are those of the launch
    return (["deep", "edges", "one", "edges", "deep"], [0, G0, 0, G0, 0],
            [(pos, base), first, (np.array([0, 0, 0]), np.array([2, 2, 3])), second, empty])


def _expected(regions):
    names, _, parts = regions
    exp = np.zeros((sum(len(p) for p in PLANTED.values()), 4), np.uint32)
    rank = {(sc, p): r for r, (sc, p) in enumerate((sc, p) for sc in PLANTED for p in PLANTED[sc])}
    for n, (pos, base) in zip(names, parts):
        sc = E_NAMES.index(n)
        k = np.array([(sc, int(p)) in rank and b < 4 for p, b in zip(pos, base)], bool)
        r = np.array([rank[(sc, int(p))] for p in pos[k]], np.int64)
        exp += np.bincount(r * 4 + base[k], minlength=exp.size).reshape(exp.shape).astype(np.uint32)
    return exp


def _send(st, regions, pick=None, shuffle=None):
    names, g0, parts = regions
    pick = range(len(names)) if pick is None else pick
    assert 0 not in pick or list(pick)[0] == 0                  # (the deep region, whose columns are aligned to the launch shape, leads)
    obs, off = [], [0]
    for i in pick:
        pos, base = parts[i]
        order = np.arange(len(pos)) if shuffle is None else shuffle.permutation(len(pos))
        obs.append(_obs(pos[order] + g0[i], base[order], np.arange(len(pos)) % 3))       # (mm is ignored)
        off.append(off[-1] + len(pos))
    st.pool_add_obs("Y", [names[i] for i in pick], np.concatenate(obs), off, gpos0=[g0[i] for i in pick])


def _counts_of(st):
    st.pooled_tables()
    return st.pool_raw["counts"].copy(), st.pool_raw["meta"].copy()


def test_pull_obs_edges_against_bincount(edges):
    st, regions = edges, _edge_regions()
    exp = _expected(regions)
    assert exp[:, :].sum() > 2000 and (exp.sum(axis=1) > 0).all()
    st.pool_sites()
    _send(st, regions)                                          # everything in one call: two regions of `edges`, an empty one
    st.pool_obs_done("Y")
    counts, meta = _counts_of(st)
    assert counts[1].tolist() == exp.tolist()
    assert counts[0].tolist() == [[10, 10, 0, 0]] * len(exp) and (meta[0] & 2).all() and not (meta[1] & 2).any()
    st.pool_sites()                                             # the same observations in another order inside every region
    _send(st, regions, shuffle=np.random.Generator(np.random.PCG64(5)))
    st.pool_obs_done("Y")
    assert _counts_of(st)[0].tobytes() == counts.tobytes()
    st.pool_sites()                                             # the same split over three calls: counts add across calls
    _send(st, regions, pick=[0, 3])
    _send(st, regions, pick=[1])
    _send(st, regions, pick=[4, 2])
    st.pool_obs_done("Y", ["deep", "one", "edges"])
    assert _counts_of(st)[0].tobytes() == counts.tobytes()
    st.pool_sites()                                             # twice the observations of a region give twice its counts
    _send(st, regions, pick=[0])
    _send(st, regions, pick=[0])
    st.pool_obs_done("Y")
    assert _counts_of(st)[0][1].tolist() == (2 * _expected((["deep"], [0], [regions[2][0]]))).tolist()


def test_no_observation_gives_zeros_and_owned_sites_stay(edges):
    st = edges
    st.pool_sites()
    st.pool_add_obs("Y", [], _obs([], []), [0])                 # n_obs = 0
    st.pool_add_obs("X", ["edges", "deep"], _obs([0, 63, 100, 100], [3, 3, 2, 2]), [0, 2, 4])       # X owns every site: nothing to add
    st.pool_obs_done("Y")
    st.pool_obs_done("X", ["edges", "deep"])
    counts, _ = _counts_of(st)
    assert not counts[1].any() and counts[0].tolist() == [[10, 10, 0, 0]] * counts.shape[1]


# ---- 4. pull by observations equals pull by batch ----
def test_pull_by_observations_equals_pull_by_batch(ctx):
    """the same reads of three pullers -- a resident one-level batch, a resident four-level batch, observations with mm left in --
    against one owner: identical count columns"""
    from instrain_amd import compare, engine
    lengths, names = [65, 700, 129], ["x", "y", "z"]
    sb = np.r_[0, np.cumsum(lengths)]
    rng = np.random.Generator(np.random.PCG64(66))
    ref = rng.integers(0, 4, int(sb[-1]))
    codes = engine.encode_seq("".join("ACTG"[i] for i in ref))
    pos = np.repeat(np.arange(sb[-1]), 12)
    obase = rng.integers(0, 4, len(pos))
    obase[pos == 300] = np.r_[np.full(6, (ref[300] + 1) % 4), np.full(6, ref[300])]               # surely a site
    owner = Sample("owner", pos, obase, np.zeros(len(pos), int), 1, sb=sb, names=names)
    ppos = np.r_[np.repeat(np.arange(sb[-1]), 12), np.full(3000, 300)]
    pmm = rng.integers(0, 4, len(ppos))
    pullers = [Sample("one", ppos, ref[ppos], pmm * 0, 1, sb=sb, names=names), Sample("four", ppos, ref[ppos], pmm, 4, sb=sb, names=names),
               Sample("obs", ppos, ref[ppos], pmm, 4, sb=sb, names=names)]
    st = compare.SampleSet(ctx, names, lengths, min_cov=5, pooling=True)
    batches = {s.name: s.batch(ctx, codes) for s in [owner] + pullers[:2]}
    for n, (b, bn, bb) in batches.items():
        st.add_batch(n, b, bn, bb)
    st.add_profile_pooled("obs", *pullers[2].stored(ctx, codes))
    assert st.pool_sites() > 600
    for n, (b, bn, bb) in batches.items():
        st.pool_add(n, b, bn, bb)
        b.close()
    _pull_obs(st, pullers[2])
    st.pooled_tables()
    c = st.pool_raw["counts"]
    st.close()
    assert c[1].tobytes() == c[2].tobytes() == c[3].tobytes() and c[1].sum() > 12 * 600 and c[3].max() >= 3012


# ---- 4b. hand-built stored rows: both row tables out of set order, a cryptic top row, every branch of the verdict ----
def _stored_row(scaffold, position, mm, ref, con, var="A", allele_count=1, counts=None, cryptic=False):
    cnt = dict(A=0, C=0, T=0, G=0)
    cnt.update(counts or {con: 20})
    return dict(scaffold=scaffold, position=position, mm=mm, ref_base=ref, con_base=con, var_base=var, allele_count=allele_count,
                **{"class": "SNS", "cryptic": cryptic}, **cnt)


def test_hand_built_rows_out_of_order_in_a_pooling_set(ctx):
    """Two samples from stored tables in a set with pooling; `a` brings its last scaffold first, so its compare rows AND its pool rows
    lie out of set order and both are sorted once.  p:10 of `a` has a cryptic row at mm 1 above a plain one at mm 0: the compare row is
    the mm 1 row, the pool row the mm 0 row; p:50 has a cryptic row only: a compare row, no pool row, no site.  On `big` (two tiles, a
    row on its last position) the two samples differ in consensus at four positions, one per branch of call_pop_snps: `b` shows a's
    consensus (5 of 30 reads; the null model asks for 3), `a` shows b's (10 of 30), both are multi-allelic with one var_base, none of
    these (the one population SNP); at position 0 they agree (no SNP).  `n` has a row at an N reference in `a` alone: the scaffold
    fails.  Every expectation below is worked out by hand from readComparer.py:292-367 and polymorpher.py:53-70."""
    from instrain_amd import compare
    lut, _ = util.load_lut()
    assert int(lut[30]) == 3 and int(lut[20]) == 2
    names, lengths = ["p", "n", "big"], [100, 70, 4097]
    full = lambda ln: (np.arange(ln), np.full(ln, 9))
    a_cov = {"p": {0: full(100), 1: (np.array([0]), np.array([1]))}, "n": {0: full(70)}, "big": {0: full(4097)}}
    b_cov = {n: {0: full(ln)} for n, ln in zip(names, lengths)}
    a_rows = pd.DataFrame([
        _stored_row("p", 10, 1, "A", "G", cryptic=True), _stored_row("p", 10, 0, "A", "C"),
        _stored_row("p", 50, 0, "A", "C", cryptic=True),
        _stored_row("n", 5, 0, "N", "A"),
        _stored_row("big", 0, 0, "A", "C"), _stored_row("big", 64, 0, "A", "C"), _stored_row("big", 2000, 0, "A", "C"),
        _stored_row("big", 4095, 0, "A", "C", counts={"C": 20, "T": 10}),
        _stored_row("big", 4096, 0, "A", "C", var="G", allele_count=2)])
    b_rows = pd.DataFrame([
        _stored_row("big", 0, 0, "A", "C"), _stored_row("big", 64, 0, "A", "T", counts={"T": 25, "C": 5}),
        _stored_row("big", 2000, 0, "A", "T"), _stored_row("big", 4095, 0, "A", "T"),
        _stored_row("big", 4096, 0, "A", "T", var="G", allele_count=2)])
    st = compare.SampleSet(ctx, names, lengths, min_cov=5, pooling=True)
    st.add_profile_pooled("a", {"big": a_cov["big"]}, a_rows, mm_values=[0, 1])
    st.add_profile_pooled("a", {"p": a_cov["p"], "n": a_cov["n"]}, a_rows, mm_values=[0, 1])
    st.add_profile_pooled("b", b_cov, b_rows)
    logs = []
    table = st.compare(min_freq=0.05, logs=logs)
    m = st.mismatch_locations("a", "b")
    assert [(r["scaffold"], r["mm"], r["consensus_SNPs"], r["population_SNPs"], r["compared_bases_count"]) for r in table] == \
        [("p", 0, 2, 2, 100), ("p", 1, 2, 2, 100), ("big", 0, 4, 1, 4097)]
    assert len(logs) == 1 and "DEBUG FAILURE CompareScaffold n ['a', 'b']" in logs[0]
    raw = m["raw"]
    got = list(zip(raw["mm"].tolist(), m["scaffold"].tolist(), m["position"].tolist(), raw["consensus_snp"].tolist(),
                   raw["population_snp"].tolist(), raw["has_a"].tolist(), raw["has_b"].tolist(), raw["con_a"].tolist(), raw["con_b"].tolist()))
    assert got == [(0, 0, 10, 1, 1, 1, 0, 3, 0), (0, 0, 50, 1, 1, 1, 0, 1, 0),
                   (0, 2, 64, 1, 0, 1, 1, 1, 2), (0, 2, 2000, 1, 1, 1, 1, 1, 2), (0, 2, 4095, 1, 0, 1, 1, 1, 2), (0, 2, 4096, 1, 0, 1, 1, 1, 2),
                   (1, 0, 10, 1, 1, 1, 0, 3, 0), (1, 0, 50, 1, 1, 1, 0, 1, 0)]
    assert raw["cnt_a"][0].tolist() == [0, 0, 0, 20] and raw["cnt_b"][2].tolist() == [0, 5, 25, 0] and raw["cnt_a"][4].tolist() == [0, 20, 10, 0]
    # pooling: the sites are the positions of the rows that are not cryptic; a owns them all, b pulls p:10 and n:5 (no reads: zeros)
    assert st.pool_sites() == 7
    off = st.offsets
    assert st.pool_site_positions().tolist() == [off[0] + 10, off[1] + 5] + [off[2] + p for p in (0, 64, 2000, 4095, 4096)]
    assert st.pool_plan("a") == {} and st.pool_plan("b") == {"p": (9, 11, 1), "n": (4, 6, 1)}
    st.pool_obs_done("b")
    st.pooled_tables()
    counts, meta = st.pool_raw["counts"], st.pool_raw["meta"]
    st.close()
    assert counts[0].tolist() == [[0, 20, 0, 0], [20, 0, 0, 0], [0, 20, 0, 0], [0, 20, 0, 0], [0, 20, 0, 0], [0, 20, 10, 0], [0, 20, 0, 0]]
    assert counts[1].tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [0, 20, 0, 0], [0, 5, 25, 0], [0, 0, 20, 0], [0, 0, 20, 0], [0, 0, 20, 0]]
    own = (meta & 2) != 0
    assert own[0].all() and own[1].tolist() == [False, False] + [True] * 5 and (meta & 1).all()
    assert ((meta[0] >> 5) & 3).tolist() == [1, 0, 1, 1, 1, 1, 1]          # con_base of a's own rows: p:10 is the mm 0 row's C, not G


# ---- 5. refusals ----
def test_refusals_leave_the_set_as_it_was(ctx, edges):
    from instrain_amd import compare, _lib
    st = edges
    st.pool_sites()
    _send(st, _edge_regions(), pick=[1])
    before = None

    def refused(code, call):
        with pytest.raises(_lib.IsxError) as e:
            call()
        assert e.value.code == code, e.value
        return str(e.value)

    def unchanged():
        n = st.n_pool_sites
        counts, meta = np.zeros((2, n, 4), np.uint32), np.zeros((2, n), np.uint8)
        for i in range(2):
            _lib.check(st.lib.isx_cmpset_pool_fetch_sample(st.h, i, counts[i].ctypes.data, meta[i].ctypes.data))
        return counts.tobytes() + meta.tobytes()
    before = unchanged()
    msg = refused(ERR_STATE, st.pooled_tables)                 # planned scaffolds are open: the first one is named, and its sample
    assert "scaffold one" in msg and "'Y'" in msg
    refused(ERR_ARG, lambda: st.pool_add_obs("Y", ["edges"], _obs([320], [0]), [0, 1]))            # beyond the scaffold
    refused(ERR_ARG, lambda: st.pool_add_obs("Y", ["edges"], _obs([999], [0]), [0, 1], gpos0=[1000]))      # before it
    refused(ERR_ARG, lambda: st.pool_add_obs("Y", ["edges"], _obs([0], [5]), [0, 1]))              # base 5
    refused(ERR_ARG, lambda: st.pool_add_obs("Y", ["edges", "deep"], _obs([0, 0], [0, 0]), [0, 2, 1]))     # descending offsets
    refused(ERR_ARG, lambda: st.pool_add_obs("Y", ["edges"], _obs([0, 0], [0, 0]), [0, 1]))        # offsets that do not end at n_obs
    ids = np.array([7], np.int32)
    z = np.zeros(2, np.int64)
    assert st.lib.isx_cmpset_pool_add_obs(st.h, 1, 1, ids.ctypes.data, z.ctypes.data, z.ctypes.data, 0, None, None) == ERR_ARG   # an id outside the set
    assert unchanged() == before
    st.pool_obs_done("Y", ["edges"])
    refused(ERR_STATE, lambda: st.pool_obs_done("Y", ["edges"]))                                   # done twice
    refused(ERR_STATE, lambda: st.pool_add_obs("Y", ["edges"], _obs([0], [0]), [0, 1]))            # observations for a closed scaffold
    assert unchanged() == before
    # a scaffold pulled by pool_add takes no observations; one with observations under way is refused by pool_add
    from instrain_amd import engine
    codes = engine.encode_seq("A" * int(E_SB[-1]))
    y = Sample("Y", np.repeat(np.arange(E_SB[-1]), 6), np.zeros(6 * int(E_SB[-1]), np.uint8), np.zeros(6 * int(E_SB[-1]), int), 1, sb=E_SB, names=E_NAMES)
    b_one, n_one, bb_one = y.batch(ctx, codes, [0])
    st.pool_add("Y", b_one, n_one, bb_one)
    after_one = unchanged()
    refused(ERR_STATE, lambda: st.pool_add_obs("Y", ["one"], _obs([0], [0]), [0, 1]))
    refused(ERR_STATE, lambda: st.pool_obs_done("Y", ["one"]))
    st.pool_add_obs("Y", ["deep"], _obs([100], [1]), [0, 1])
    b_deep, n_deep, bb_deep = y.batch(ctx, codes, [2])
    under_way = unchanged()
    assert under_way != after_one
    refused(ERR_STATE, lambda: st.pool_add("Y", b_deep, n_deep, bb_deep))
    msg = refused(ERR_STATE, st.pooled_tables)                 # `one` and `edges` are pulled: the scaffold with observations under way
    assert "scaffold deep" in msg and "isx_cmpset_pool_obs_done" in msg
    assert unchanged() == under_way
    b_one.close()
    b_deep.close()
    # before pool_sites; without pooling; flags
    fresh = compare.SampleSet(ctx, E_NAMES, E_LENGTHS, min_cov=5, pooling=True)
    cov = {"edges": {0: (np.arange(320), np.full(320, 6))}}
    row = pd.DataFrame([{"scaffold": "edges", "position": 5, "mm": 0, "con_base": "A", "ref_base": "A", "var_base": "C", "allele_count": 2,
                         "A": 5, "C": 5, "T": 0, "G": 0, "class": "SNV", "cryptic": False}])
    fresh.add_profile_pooled("a", cov, row)
    fresh.add_profile_pooled("b", cov, pd.DataFrame())
    refused(ERR_STATE, lambda: fresh.pool_add_obs("a", ["edges"], _obs([0], [0]), [0, 1]))         # before pool_sites
    refused(ERR_STATE, lambda: fresh.pool_obs_done("a", ["edges"]))
    refused(ERR_STATE, lambda: fresh.add_profile("c", cov))                                        # the pinned refusal, again
    assert fresh.samples == ["a", "b"]
    assert fresh.pool_sites() == 1
    p = compare.pack_profile(fresh.index, fresh.lengths, cov, row, pool=True)
    for bad in (0x10 | 3, 7, 6):
        fl = np.array([bad], np.uint8)
        ms = _lib.C.c_float(0)
        rc = fresh.lib.isx_cmpset_add_profile_pool(fresh.h, 2, 1, p["ids"].ctypes.data, 1, p["levels"].ctypes.data, p["present"].ctypes.data,
                                                   p["offsets"].ctypes.data, p["positions"].ctypes.data, p["values"].ctypes.data, 1,
                                                   p["snv"].ctypes.data, fl.ctypes.data, _lib.C.byref(ms))
        assert rc == ERR_ARG, bad
    assert fresh.n_pool_sites == 1 and fresh.pool_plan("b") == {"edges": (4, 6, 1)}              # (the refused adds dropped nothing)
    plain = compare.SampleSet(ctx, E_NAMES, E_LENGTHS, min_cov=5)
    refused(ERR_STATE, lambda: plain.add_profile_pooled("a", cov, row))
    ms = _lib.C.c_float(0)
    assert plain.lib.isx_cmpset_add_profile_pool(plain.h, 0, 1, p["ids"].ctypes.data, 1, p["levels"].ctypes.data, p["present"].ctypes.data,
                                                 p["offsets"].ctypes.data, p["positions"].ctypes.data, p["values"].ctypes.data, 1,
                                                 p["snv"].ctypes.data, p["flags"].ctypes.data, _lib.C.byref(ms)) == ERR_STATE
    assert plain.samples == []
    plain.add_profile("a", cov, row)                            # and it still takes what it should
    fresh.close()
    plain.close()


# ---- 6. from BAM files: live == stored + pool_stored == stored + profile_bam(pool_set=) ----
B_REFS = [("ctgA", 300), ("ctgB", 400), ("ctgC", 250)]
B_FLAGS = dict(min_read_ani=0.95, min_mapq=-1, max_insert_relative=3, min_insert=50, pairing_filter="paired_only")
# sample -> {(scaffold index, position): alternative-base shift}; s2 has no read on ctgC; (0, 100) is called by s0 alone
B_VARIANTS = {"s0": {(0, 100): 1, (1, 200): 1, (2, 120): 2}, "s1": {(1, 200): 2, (1, 201): 1, (2, 120): 2}, "s2": {(1, 30): 3, (1, 200): 1}}
B_JUNK = {"s1": (0, 100), "s2": (0, 100)}           # pairs far below the read-ANI cut that carry a third base over s0's own site


def _write_sample(path, name, ref_codes):
    """clean 50-base pairs (50M, mate 60 further on) every 2 positions; every other pair carries the sample's alternative bases; NM says
    how many.  The junk pairs of B_JUNK carry 7 mismatches a read (ANI 0.86): the filter must drop them"""
    from tests import bamwriter
    letters = "ACTG"
    reads = []

    def add(tid, s, pname, alts):
        for mate, start in enumerate((s, s + 60)):
            codes = ref_codes[tid][start:start + 50].copy()
            nm = 0
            for p, shift in alts.items():
                if start <= p < start + 50:
                    codes[p - start] = (codes[p - start] + shift) % 4
                    nm += 1
            reads.append(dict(tid=tid, pos=start, mapq=40, flag=0x1 | 0x2 | (0x40 | 0x20 if mate == 0 else 0x80 | 0x10), name=pname, cigar=[("M", 50)],
                              seq="".join(letters[c] for c in codes), qual=np.full(50, 40), nm=nm, isize=110 if mate == 0 else -110))
    for tid, (_, ln) in enumerate(B_REFS):
        if name == "s2" and tid == 2:
            continue
        alts = {p: sh for (t, p), sh in B_VARIANTS[name].items() if t == tid}
        for k, s in enumerate(range(0, ln - 110, 2)):
            add(tid, s, "%s_%d_%d" % (name, tid, k), alts if k % 2 else {})
    if name in B_JUNK:
        tid, p = B_JUNK[name]
        for k in range(6):
            s = p - 20 - k
            junk = {p: 3}
            junk.update({s + j: 1 for j in range(0, 12, 2)})
            junk.update({s + 60 + j: 1 for j in range(0, 14, 2)})
            add(tid, s, "%s_junk_%d" % (name, k), junk)
    reads.sort(key=lambda r: (r["tid"], r["pos"]))
    bamwriter.write_bam(path, B_REFS, reads)


@pytest.fixture(scope="module")
def bams(ctx, tmp_path_factory):
    """three BAMs; every sample profiled live into set L (own rows, then the pull), its profile stored and loaded again"""
    import instrain_amd.profile as prof
    from instrain_amd import compare
    lut, fb = util.load_lut()
    model = {int(i): int(v) for i, v in enumerate(lut) if v >= 0}
    model[-1] = fb
    rng = np.random.Generator(np.random.PCG64(606))
    ref_codes = [rng.integers(0, 4, ln) for _, ln in B_REFS]
    s2s = {n: "".join("ACTG"[c] for c in codes) for (n, _), codes in zip(B_REFS, ref_codes)}
    tmp = tmp_path_factory.mktemp("pool_bams")
    names, lengths = [n for n, _ in B_REFS], [ln for _, ln in B_REFS]
    kw = dict(s2s=s2s, null_model=model, min_cov=5, min_freq=0.05, min_snp=20, ctx=ctx, **B_FLAGS)
    L = compare.SampleSet(ctx, names, lengths, min_cov=5, pooling=True)
    name2bam, loaded = {}, {}
    for s in ("s0", "s1", "s2"):
        name2bam[s] = str(tmp / (s + ".bam"))
        _write_sample(name2bam[s], s, ref_codes)
        splits = prof.profile_bam(name2bam[s], compare_set=L, compare_sample=s, **kw)
        folder = str(tmp / s / "raw_data")
        compare.store_sample(folder, splits)
        loaded[s] = compare.load_sample(folder)
    assert L.pool_sites() > 0
    for s in name2bam:
        prof.profile_bam(name2bam[s], pool_set=L, pool_sample=s, **kw)
    dst, pm = L.pooled_tables()
    L.close()
    return dict(names=names, lengths=lengths, name2bam=name2bam, loaded=loaded, dst=dst, pm=pm, kw=kw, ref_codes=ref_codes)


def _stored_set(ctx, bams):
    from instrain_amd import compare
    S = compare.SampleSet(ctx, bams["names"], bams["lengths"], min_cov=5, pooling=True)
    for s, (covT, table) in bams["loaded"].items():
        S.add_profile_pooled(s, covT, table)
    assert S.pool_sites() == len(bams["pm"])
    return S


def _same_tables(S, bams):
    dst, pm = S.pooled_tables()
    pool_ref.same_frames(dst, bams["dst"])
    pool_ref.same_frames(pm, bams["pm"])


def test_bam_live_tables_hold_what_the_case_needs(bams):
    dst, pm = bams["dst"], bams["pm"]
    A = dst[dst["scaffold"] == "ctgA"]
    assert (pm["scaffold"] == "ctgA").sum() == 1 and pm[pm["scaffold"] == "ctgA"].index[0] == 100               # the site s0 alone calls
    assert set(A.index.get_level_values(0)) == {"s0", "s1", "s2"}
    assert "s2" not in set(dst[dst["scaffold"] == "ctgC"].index.get_level_values(0)) and (pm["scaffold"] == "ctgC").any()
    junk = "ACTG"[(bams["ref_codes"][0][100] + 3) % 4]       # the base only the filtered pairs carry there
    assert int(A[junk].sum()) == 0 and int(A.loc["s1"][["A", "C", "T", "G"]].to_numpy().sum()) > 20
    assert all("class" in t.columns and "cryptic" in t.columns and len(t) > 0 for _, t in bams["loaded"].values())


def test_bam_pool_stored_equals_live(ctx, bams):
    from instrain_amd import compare
    S = _stored_set(ctx, bams)
    stats = compare.pool_stored(S, bams["name2bam"], **B_FLAGS)
    assert set(stats) == {"s0", "s1", "s2"} and all(v["windows"] == v["scaffolds"] > 0 and v["observations"] > 0 for v in stats.values())
    _same_tables(S, bams)
    S.close()
    # without the read-ANI cut the junk pairs count: the filter is what makes the tables equal
    S = _stored_set(ctx, bams)
    compare.pool_stored(S, bams["name2bam"], **dict(B_FLAGS, min_read_ani=0.5))
    dst, _ = S.pooled_tables()
    S.close()
    junk = "ACTG"[(bams["ref_codes"][0][100] + 3) % 4]
    assert int(dst[dst["scaffold"] == "ctgA"][junk].sum()) == 12


def test_bam_stored_set_pulled_by_profile_bam_equals_live(ctx, bams):
    import instrain_amd.profile as prof
    P = _stored_set(ctx, bams)
    for s, path in bams["name2bam"].items():
        prof.profile_bam(path, pool_set=P, pool_sample=s, **bams["kw"])
    _same_tables(P, bams)
    P.close()


def test_bam_pool_stored_with_r2m_and_in_several_windows(ctx, bams):
    from instrain_amd import compare, engine
    name2r2m = {}
    for s, path in bams["name2bam"].items():
        bf = engine.BamFile(path)
        bf.scan()
        bf.filter(**B_FLAGS)
        name2r2m[s] = {n: bf.r2m(tid) for tid, (n, _, _) in enumerate(bf.refs())}
        bf.close()
    assert all(not any("junk" in p for p in m) for d in name2r2m.values() for m in d.values()) and len(name2r2m["s0"]["ctgA"]) > 50
    S = _stored_set(ctx, bams)
    compare.pool_stored(S, bams["name2bam"], name2r2m=name2r2m, min_read_ani=0.5)       # (the flags would let the junk pairs in: R2M decides)
    _same_tables(S, bams)
    S.close()
    S = _stored_set(ctx, bams)
    stats = compare.pool_stored(S, bams["name2bam"], max_obs=40, **B_FLAGS)               # (fewer than one column of ~46 reads holds)
    assert all(v["windows"] > v["scaffolds"] for v in stats.values())
    _same_tables(S, bams)
    S.close()
