"""GPU: SNV pooling over a sample set (compare.SampleSet(pooling=True): isx_cmpset_pool_*) against the reference's own DSTdb / PMdb
(tests/golden/make_pool_golden.py) and against tests/pool_ref.py, the numpy / pandas restatement that test_pool_ref.py holds against the
same golden tables.  Every compared value is an integer or a string: equality throughout."""
import os
import re

import numpy as np
import pytest

from tests import pool_ref, util

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LENGTHS = [1, 63, 64, 65, 127, 128, 129, 4096, 4097]         # word edges, a scaffold inside one word, 64 words and one position more
NAMES = ["sc%d" % i for i in range(len(LENGTHS))]
SB = np.r_[0, np.cumsum(LENGTHS)]
ERR_STATE = -6


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
    b = engine.Batch(ctx, codes, bounds, engine.pack_obs(np.asarray(pos).astype(np.uint32), np.asarray(base).astype(np.uint8), mm),
                     np.arange(len(pos), dtype=np.uint32), n_mm_bins=n_mm, enable_linkage=False)
    b.run()
    return b


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
        for sc in drop:                                          # no read at all on these scaffolds
            keep &= ~((pos >= SB[sc]) & (pos < SB[sc + 1]))
        return cls(name, pos[keep], base[keep], mm[keep] if n_levels > 1 else mm[keep] * 0, n_levels, values)

    def arrays(self, codes, scaffolds=None):
        """the observations on the given scaffolds, in the given order (None: all, set order), as a flat space of their own"""
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
        return ref, bounds, new_pos, self.base[sel], self.mm[sel], [self.names[sc] for sc in scaffolds]

    def batch(self, ctx, codes, scaffolds=None):
        ref, bounds, pos, base, mm, names = self.arrays(codes, scaffolds)
        return _batch(ctx, ref, bounds, pos, base, mm, self.n_levels), names, bounds

    def observations(self):
        return (self.name, self.pos, self.base, self.real_mm)


def _pool(ctx, names, lengths, codes, samples, pieces=None):
    """the whole flow on resident batches -> (DSTdb, PMdb, the device's bytes, site positions).  pieces[name]: scaffold lists the
    sample comes in, for the add and again for the pull"""
    from instrain_amd import compare
    st = compare.SampleSet(ctx, names, lengths, min_cov=5, pooling=True)
    parts = lambda s: (pieces or {}).get(s.name, [None])
    for s in samples:
        for part in parts(s):
            b, bn, bb = s.batch(ctx, codes, part)
            st.add_batch(s.name, b, bn, bb, mm_values=s.values)
            b.close()
    n = st.pool_sites()
    sites = st.pool_site_positions()
    for s in samples:
        for part in reversed(parts(s)):
            b, bn, bb = s.batch(ctx, codes, part)
            st.pool_add(s.name, b, bn, bb)
            b.close()
    dst, pm = st.pooled_tables()
    raw = b"".join(st.pool_raw[k].tobytes() for k in ("summary", "counts", "meta")) + sites.tobytes()
    assert len(pm) == n == len(sites) and st.pool_device_ms > 0
    st.close()
    return dst, pm, raw, sites


# ---- 1. the reference's tables through the device ----
def test_golden_through_the_device(ctx):
    from instrain_amd import engine
    g = np.load(os.path.join(GOLDEN, "pool_obs.npz"))
    names, lengths = [str(n) for n in g["names"]], g["lengths"].tolist()
    sb = np.r_[0, np.cumsum(lengths)]
    codes = engine.encode_seq(str(g["seq"]))
    samples = [Sample(str(s), g[str(s) + "_pos"], g[str(s) + "_base"], g[str(s) + "_mm"], int(g[str(s) + "_mm"].max()) + 1, sb=sb, names=names)
               for s in g["samples"]]
    dst, pm, _, _ = _pool(ctx, names, lengths, codes, samples)
    exp_dst, exp_pm = pool_ref.load_golden(GOLDEN, names)
    pool_ref.same_frames(dst, exp_dst)
    pool_ref.same_frames(pm, exp_pm)


# ---- 2. - 4. five samples against the restatement; in pieces; twice ----
@pytest.fixture(scope="module")
def five(ctx):
    from instrain_amd import engine
    from tests.test_gpu_parity import _random_split
    seq = re.sub("[^ACGT]", "A", _random_split(700, int(SB[-1]), 5, 1, 10)[0])
    codes = engine.encode_seq(seq)
    samples = [Sample.random("s0", 701, 30, 1), Sample.random("s1", 702, 24, 1, drop=(3, 7)), Sample.random("s2", 703, 26, 4),
               Sample.random("s3", 704, 28, 3, values=[0, 1, 3]), Sample.random("s4", 705, 22, 2, values=[0, 2])]
    dst, pm, raw, _ = _pool(ctx, NAMES, LENGTHS, codes, samples)
    return dict(seq=seq, codes=codes, samples=samples, dst=dst, pm=pm, raw=raw)


def test_five_samples_vs_restatement(five):
    lut, fb = util.load_lut()
    exp_dst, exp_pm = pool_ref.pooled_tables([s.observations() for s in five["samples"]], five["seq"], NAMES, LENGTHS, lut, fb)
    pool_ref.same_frames(five["dst"], exp_dst)
    pool_ref.same_frames(five["pm"], exp_pm)
    pm, dst = five["pm"], five["dst"]
    # not vacuous: sites on the big scaffolds, pulled rows, a sample without a scaffold, more than one con_base somewhere
    assert len(pm) > 50 and {"sc7", "sc8"} <= set(pm["scaffold"]) and (pm["sample_detections"] > pm[[c for c in pm if c.endswith("_count")]].sum(axis=1)).any()
    assert "s1" not in set(dst[dst["scaffold"] == "sc7"].index.get_level_values(0)) and "s1" in set(dst[dst["scaffold"] == "sc8"].index.get_level_values(0))
    assert pm["sample_con_bases"].str.contains(" ").any()


def test_a_sample_in_pieces(ctx, five):
    """every sample added and pulled in two batches that cut the scaffold list at different places, in another scaffold order (the pull in
    yet another order of the pieces): byte-identical fetches -- the pool rows are sorted once, sites and ranks do not depend on arrival"""
    order = [[5, 2, 8, 0, 7, 1, 4, 6, 3], [8, 7, 6, 5, 4, 3, 2, 1, 0], [3, 0, 4, 8, 1, 7, 2, 6, 5], [1, 8, 0, 2, 3, 4, 5, 6, 7],
             [6, 4, 7, 3, 8, 5, 0, 1, 2]]
    pieces = {s.name: [order[k][2 + k:], order[k][:2 + k]] for k, s in enumerate(five["samples"])}
    dst, pm, raw, _ = _pool(ctx, NAMES, LENGTHS, five["codes"], five["samples"], pieces=pieces)
    assert raw == five["raw"]
    pool_ref.same_frames(dst, five["dst"])
    pool_ref.same_frames(pm, five["pm"])


def test_two_runs_give_identical_bytes(ctx, five):
    _, _, raw, _ = _pool(ctx, NAMES, LENGTHS, five["codes"], five["samples"])
    assert raw == five["raw"] and len(raw) > 0


# ---- 5. plane and rank edges ----
def test_plane_and_rank_edges(ctx):
    """an all-A reference; sample X shows {A, C} at the planted sites and A elsewhere, sample Y shows A everywhere.  Sites at bits 0 and 63
    of the first and last word of a scaffold, a full word between empty ones and next to a full one, a 300 000-position scaffold
    (4 688 words) with sites only in its first and last word, a scaffold of length 1 that is a site"""
    from instrain_amd import compare, engine
    lengths = [1, 320, 256, 300000, 1]
    names = ["one", "edges", "full", "long", "last"]
    sb = np.r_[0, np.cumsum(lengths)]
    planted = {0: [0], 1: [0, 63, 256, 319], 2: list(range(64, 192)), 3: [0, 63, 299968, 299999], 4: []}
    codes = engine.encode_seq("A" * int(sb[-1]))
    # coverage: everywhere on the short scaffolds, the first and last 64 positions of the long one
    covered = np.concatenate([np.arange(sb[sc], sb[sc + 1]) if lengths[sc] < 1000 else np.r_[sb[sc]:sb[sc] + 64, sb[sc + 1] - 64:sb[sc + 1]]
                              for sc in range(len(lengths))])
    sites = np.concatenate([sb[sc] + np.array(p, np.int64) for sc, p in planted.items()])
    is_site = np.isin(covered, sites)
    y_pos = np.repeat(covered, 6)
    x_pos = np.concatenate([np.repeat(covered[~is_site], 6), np.repeat(covered[is_site], 20)])
    x_base = np.concatenate([np.zeros(6 * int((~is_site).sum()), np.uint8), np.tile(np.r_[np.zeros(10, np.uint8), np.ones(10, np.uint8)], int(is_site.sum()))])
    X = Sample("X", x_pos, x_base, np.zeros(len(x_pos), np.int64), 1, sb=sb, names=names)
    Y = Sample("Y", y_pos, np.zeros(len(y_pos), np.uint8), np.zeros(len(y_pos), np.int64), 1, sb=sb, names=names)
    dst, pm, _, got_sites = _pool(ctx, names, lengths, codes, [X, Y])
    offsets = compare.set_layout(lengths) * 64
    exp = np.concatenate([offsets[sc] + np.array(p, np.int64) for sc, p in planted.items()])
    assert got_sites.tolist() == exp.tolist() and len(exp) == 1 + 4 + 128 + 4
    assert pm.index.tolist() == [p for sc in planted for p in planted[sc]]
    assert pm["scaffold"].astype(str).tolist() == [names[sc] for sc in planted for _ in planted[sc]] and list(pm["scaffold"].cat.categories) == names[:4]
    assert (pm["A"] == 16).all() and (pm["C"] == 10).all() and (pm["depth"] == 26).all() and (pm["sample_detections"] == 2).all()
    assert (pm["sample_con_bases"] == "['A']").all() and (pm["con_base"] == "A").all() and (pm["var_base"] == "C").all() and (pm["ref_base"] == "A").all()
    assert dst.loc["X"][["A", "C", "T", "G"]].to_numpy().tolist() == [[10, 10, 0, 0]] * len(exp)
    assert dst.loc["Y"][["A", "C", "T", "G"]].to_numpy().tolist() == [[6, 0, 0, 0]] * len(exp)
    assert dst.loc["Y"].index.tolist() == pm.index.tolist()


# ---- 6. where the pulled counts come from ----
def _deep_sample(name, seed, n_levels, lengths, hot=None, per_level=3):
    """every position `per_level * n_levels` reads deep with every level present; `hot`: one position 5000 reads deeper"""
    rng = np.random.Generator(np.random.PCG64(seed))
    n = int(np.sum(lengths))
    pos = np.repeat(np.arange(n), per_level * n_levels)
    mm = np.tile(np.repeat(np.arange(n_levels), per_level), n)
    if hot is not None:
        pos, mm = np.r_[pos, np.full(5000, hot)], np.r_[mm, rng.integers(0, n_levels, 5000)]
    return name, pos, rng.integers(0, 4, len(pos)).astype(np.uint8), mm


def test_sources_of_counts(ctx):
    """one owner of many sites (random bases: nearly every position is a site) and, pulled against it, the same observations through
    a resident one-level batch, a resident 4-level batch with a 5000-deep position, a resident 6-level batch whose windows hold more
    (position, level) entries than their slabs (4 per position) so that the rest lies in the overflow region, a one-level pipe with
    want_counts and a 4-level pipe (flat level table).  A one-level pipe without a count table is refused and changes nothing."""
    from instrain_amd import compare, engine
    from instrain_amd._lib import IsxError
    lengths, names = [65, 700, 129], ["x", "y", "z"]
    sb = np.r_[0, np.cumsum(lengths)]
    rng = np.random.Generator(np.random.PCG64(66))
    seq = "".join("ACTG"[i] for i in rng.integers(0, 4, int(sb[-1])))
    codes = engine.encode_seq(seq)
    ref_codes = np.array(["ACTG".index(c) for c in seq], np.uint8)
    owner = Sample(*_deep_sample("owner", 1, 1, lengths, per_level=12), 1, sb=sb, names=names)
    owner.base[owner.pos == 300] = np.r_[np.full(6, (ref_codes[300] + 1) % 4), np.full(6, ref_codes[300])]        # surely a site
    # pullers: reads of the reference base only (they own nothing), so every site of theirs is pulled
    def puller(name, n_levels, hot=None):
        _, pos, _, mm = _deep_sample(name, 2, n_levels, lengths, hot)
        return Sample(name, pos, ref_codes[pos], mm, n_levels, sb=sb, names=names)
    pullers = [puller("one", 1), puller("four", 4, hot=300), puller("six", 6), puller("pipe1", 1), puller("pipe4", 4)]
    assert all(len(np.unique(p.mm[p.pos == q])) == p.n_levels for p in pullers for q in (0, 400, int(sb[-1]) - 1))
    st = compare.SampleSet(ctx, names, lengths, min_cov=5, pooling=True)
    pipes = {}

    def through(s, call):
        if not s.name.startswith("pipe"):
            b, bn, bb = s.batch(ctx, codes)
            call(s.name, b, bn, bb)
            b.close()
            return
        ref, bounds, pos, base, mm, bn = s.arrays(codes)
        if s.name not in pipes:
            pipes[s.name] = engine.Pipe(ctx, max_pos=int(sb[-1]), max_obs=len(pos), max_splits=16, depth=1, host_threads=2,
                                        n_mm_bins=s.n_levels, want_counts=s.n_levels == 1)
        t = pipes[s.name].submit(ref, bounds, engine.pack_obs(pos.astype(np.uint32), base, mm), np.arange(len(pos), dtype=np.uint32))
        res = pipes[s.name].collect(t)
        try:
            call(s.name, res["slot"], bn, bounds)
        finally:
            pipes[s.name].release(t)
    everyone = [owner] + pullers
    for s in everyone:
        through(s, lambda *a: st.add_batch(*a))
    n = st.pool_sites()
    assert n > 600
    # a one-level slot without a count table: refused on the host, the set stays as it was
    bare = engine.Pipe(ctx, max_pos=int(sb[-1]), max_obs=len(pullers[3].pos), max_splits=16, depth=1, host_threads=2, n_mm_bins=1)
    ref, bounds, pos, base, mm, bn = pullers[3].arrays(codes)
    t = bare.submit(ref, bounds, engine.pack_obs(pos.astype(np.uint32), base, mm), np.arange(len(pos), dtype=np.uint32))
    res = bare.collect(t)
    with pytest.raises(IsxError) as e:
        st.pool_add("pipe1", res["slot"], bn, bounds)
    assert e.value.code == ERR_STATE and "want_counts" in str(e.value)
    bare.release(t)
    bare.close()
    for s in everyone:
        through(s, lambda *a: st.pool_add(*a))
    for p in pipes.values():
        p.close()
    dst, pm = st.pooled_tables()
    st.close()
    lut, fb = util.load_lut()
    exp_dst, exp_pm = pool_ref.pooled_tables([s.observations() for s in everyone], seq, names, lengths, lut, fb)
    pool_ref.same_frames(dst, exp_dst)
    pool_ref.same_frames(pm, exp_pm)
    assert int(dst.loc["four"].loc[300 - 65, ["A", "C", "T", "G"]].to_numpy().sum()) == 5012 and len(pipes) == 2       # (3 x 4 + 5000 reads)


# ---- 7. more samples than one byte of detections, the sample loop ----
def test_seventy_samples_vs_restatement(ctx):
    """70 samples on three tiny scaffolds: the summary's loop over samples, insertion order of sample_con_bases"""
    from instrain_amd import engine
    lengths, names = [65, 1, 40], ["x", "y", "z"]
    sb = np.r_[0, np.cumsum(lengths)]
    rng = np.random.Generator(np.random.PCG64(7070))
    seq = "".join("ACTG"[i] for i in rng.integers(0, 4, int(sb[-1])))
    codes = engine.encode_seq(seq)
    samples = []
    for k in range(70):
        pos = rng.integers(0, sb[-1], size=int(sb[-1]) * 9)
        if k % 5 == 3:
            pos = pos[pos != sb[1]]                              # no read on the one-position scaffold
        base = np.array(["ACTG".index(c) for c in seq], np.uint8)[pos]
        odd = rng.random(len(pos)) < 0.15                        # enough other bases for own rows with various con_bases
        base[odd] = rng.integers(0, 4, int(odd.sum()))
        samples.append(Sample("t%d" % k, pos, base, np.zeros(len(pos), np.int64), 1, sb=sb, names=names))
    dst, pm, _, _ = _pool(ctx, names, lengths, codes, samples)
    lut, fb = util.load_lut()
    exp_dst, exp_pm = pool_ref.pooled_tables([s.observations() for s in samples], seq, names, lengths, lut, fb)
    pool_ref.same_frames(dst, exp_dst)
    pool_ref.same_frames(pm, exp_pm)
    assert pm["sample_detections"].max() > 64 and pm["sample_con_bases"].str.contains(" ").any() and len(pm) > 20


# ---- 8. state errors ----
def test_state_errors(ctx, five):
    from instrain_amd import compare
    from instrain_amd._lib import IsxError, check
    samples, codes = five["samples"][:3], five["codes"]

    def refused(call):
        with pytest.raises(IsxError) as e:
            call()
        assert e.value.code == ERR_STATE, e.value
    st = compare.SampleSet(ctx, NAMES, LENGTHS, min_cov=5, pooling=True)
    plain = compare.SampleSet(ctx, NAMES, LENGTHS, min_cov=5)
    batches = [s.batch(ctx, codes) for s in samples]
    for s, (b, bn, bb) in zip(samples, batches):
        st.add_batch(s.name, b, bn, bb, mm_values=s.values)
        plain.add_batch(s.name, b, bn, bb, mm_values=s.values)
    refused(lambda: check(st.lib.isx_cmpset_pool_enable(st.h)))                         # after an add
    b, bn, bb = batches[0]
    refused(lambda: st.pool_add("s0", b, bn, bb))                                       # before pool_sites
    refused(lambda: st.pooled_tables())
    n = st.pool_sites()
    assert n > 0
    st.pool_add("s0", b, bn, bb)
    refused(lambda: st.pool_add("s0", b, bn, bb))                                       # the same (sample, scaffold) twice
    with pytest.raises(IsxError) as e:                                                  # s1 and s2 still have sites to pull
        st.pooled_tables()
    assert e.value.code == ERR_STATE and "sample 1" in str(e.value)
    # an add after pool_sites drops the pooling state; a fresh pool_sites works
    extra = five["samples"][3]
    xb, xn, xbb = extra.batch(ctx, codes)
    st.add_batch(extra.name, xb, xn, xbb, mm_values=extra.values)
    refused(lambda: st.pool_add("s1", batches[1][0], batches[1][1], batches[1][2]))
    refused(lambda: st.pooled_tables())
    assert st.pool_sites() >= n
    for s, (b2, bn2, bb2) in zip(list(samples) + [extra], batches + [(xb, xn, xbb)]):
        st.pool_add(s.name, b2, bn2, bb2)
    dst, pm = st.pooled_tables()
    lut, fb = util.load_lut()
    exp_dst, exp_pm = pool_ref.pooled_tables([s.observations() for s in list(samples) + [extra]], five["seq"], NAMES, LENGTHS, lut, fb)
    pool_ref.same_frames(dst, exp_dst)
    pool_ref.same_frames(pm, exp_pm)
    # a set without pooling refuses every pool call; its compare() bytes equal the pooled set's
    refused(plain.pool_sites)
    refused(lambda: plain.pool_add("s0", b, bn, bb))
    refused(plain.pooled_tables)
    refused(plain.pool_site_positions)
    plain.add_batch(extra.name, xb, xn, xbb, mm_values=extra.values)
    plain.compare()
    st.compare()
    assert plain.levels.tobytes() == st.levels.tobytes() and plain.levels.size > 0
    for x in [t[0] for t in batches] + [xb]:
        x.close()
    st.close()
    plain.close()
