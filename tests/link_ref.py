"""Observation batches built for the linkage chain's edges (tests/test_gpu_link_edges.py, tests/test_link_ref.py), and the counting of
calc_mm_SNV_linkage_network restated in plain Python.  numpy / Python only: nothing here imports the product.

A "read pair" of an observation batch is a label on observations, so a case says exactly which pair sees which site with which base
and mm.  Sites k = 0..K-1 sit at positions 5 + 3k of an all-A reference; every site gets background observations (bgA of base A, bgC
of base C, a pair id each, mm 0) that make it a called SNP site with the alleles {A, C}; "linking" pairs then observe chosen
(site, base) lists with ONE mm per pair (the reference's R2M is per read pair; the kernels take the mm of whichever observation walks).

restate(): per split and pair, itertools.combinations of its allele observations in (site, arrival) order (linkage.py:26-42) -> the
increments, unique keys and edges of every first site -- what a case is asserted to sit on before the device sees it.
ld_replay(): r2 and D' of one count table in Python floats, in the reference's operation order (linkage.py:160-196)."""
import itertools
from collections import Counter, defaultdict

import numpy as np

SITE0, STEP = 5, 3
AC = (0, 1)


def site_pos(k):
    return SITE0 + STEP * k


class Builder:
    """K sites; bg(k) -> the background counts [A, C, T, G] of site k (default [bgA, bgC, 0, 0]); bases(k) -> the site's `bases` set
    (consensus and variant base of the called site), (A, C) unless `site_bases` says otherwise"""

    def __init__(self, K, bgA=30, bgC=30, bg=None, tail=5):
        self.K = K
        self.n_pos = site_pos(K - 1) + 1 + tail
        self.pos, self.base, self.mm, self.pair = [], [], [], []
        self.n_pairs = 0
        self.site_bases = {}
        for k in range(K):
            cnt = bg(k) if bg is not None else (bgA, bgC, 0, 0)
            for b, n in enumerate(cnt):
                for _ in range(n):
                    self.link([(k, b)])

    def link(self, obs, mm=0):
        """one pair observing [(site, base), ...] in this order, all at level mm -> its id"""
        p = self.n_pairs
        self.n_pairs += 1
        for k, b in obs:
            self.pos.append(site_pos(k)); self.base.append(b); self.mm.append(mm); self.pair.append(p)
        return p

    def plan(self, s1, n, u, M, edge_first=False):
        """first site s1 gets exactly n increments over u unique keys (s2, mm, b1, b2): one two-site pair per increment, cycling through
        the keys; keys enumerated s2-major, then mm, b1, b2 (edge_first: u different second sites instead)"""
        keys = plan_keys(s1, u, M, self.K, edge_first)
        for i in range(n):
            s2, mm, b1, b2 = keys[i % u]
            self.link([(s1, b1), (s2, b2)], mm)

    def arrays(self, split_bounds=None, pair_ids=None):
        """-> the batch: observations stable-sorted by position (arrival order inside a column = the order they were added)"""
        pos = np.asarray(self.pos, dtype=np.int64)
        o = np.argsort(pos, kind="stable")
        pair = np.asarray(self.pair, dtype=np.int64)[o]
        if pair_ids is not None:
            pair = np.asarray(pair_ids, dtype=np.int64)[pair]
        sb = [0, self.n_pos] if split_bounds is None else split_bounds
        return {"n_pos": self.n_pos, "ref_codes": np.zeros(self.n_pos, dtype=np.uint8), "split_bounds": np.asarray(sb, dtype=np.int64),
                "gpos": pos[o], "base": np.asarray(self.base, dtype=np.uint8)[o], "mm": np.asarray(self.mm, dtype=np.int64)[o],
                "pair": pair.astype(np.uint32), "K": self.K,
                "site_bases": {site_pos(k): v for k, v in self.site_bases.items()}}


def plan_keys(s1, u, M, K, edge_first=False):
    if edge_first:
        assert s1 + u < K, "an edge-first plan needs u later sites"
        return [(s1 + 1 + i, 0, 0, 0) for i in range(u)]
    keys = []
    for s2 in range(s1 + 1, K):
        for mm in range(M):
            for b1 in AC:
                for b2 in AC:
                    keys.append((s2, mm, b1, b2))
                    if len(keys) == u:
                        return keys
    raise AssertionError("not enough later sites for %d keys behind site %d" % (u, s1))


def restate(w):
    """the counting of calc_mm_SNV_linkage_network on a batch of arrays(): dict with n_allele_obs, n_sites, n_increments, n_edges,
    keys (Counter of (split, p1, p2, mm, b1, b2)), per_site {(split, p1): (increments, unique keys, edges)}"""
    gpos, base, mm, pair = w["gpos"], w["base"], w["mm"], w["pair"]
    split = np.searchsorted(w["split_bounds"], gpos, side="right") - 1
    sbases = w.get("site_bases", {})
    lists = defaultdict(list)
    n_ao, sites = 0, set()
    for g, b, m, p, s in zip(gpos.tolist(), base.tolist(), mm.tolist(), pair.tolist(), split.tolist()):
        if b in sbases.get(g, AC):
            lists[(s, p)].append((g, b, m))
            n_ao += 1
            sites.add(g)
    keys = Counter()
    for (s, _), lst in lists.items():
        if len(lst) > 1:
            for (p1, b1, m1), (p2, b2, _m2) in itertools.combinations(lst, 2):
                keys[(s, p1, p2, m1, b1, b2)] += 1
    inc, nu, edges = Counter(), Counter(), defaultdict(set)
    for (s, p1, p2, m, b1, b2), c in keys.items():
        inc[(s, p1)] += c
        nu[(s, p1)] += 1
        edges[(s, p1)].add(p2)
    per_site = {k: (inc[k], nu[k], len(edges[k])) for k in inc}
    return {"n_allele_obs": n_ao, "n_sites": len(sites), "n_increments": sum(inc.values()), "n_edges": sum(len(e) for e in edges.values()),
            "keys": keys, "per_site": per_site}


def site_shape(r, k, split=0):
    """(increments, unique keys, edges) of first site k in restate()'s result"""
    return r["per_site"].get((split, site_pos(k)), (0, 0, 0))


def ld_replay(AB, Ab, aB, ab):
    """(r2, D') of a pair table as the reference computes them: Python floats, its operation order (linkage.py:160-196)"""
    total = AB + Ab + aB + ab
    t = float(total)
    fAB, fAb, faB, fab = AB / t, Ab / t, aB / t, ab / t
    fA, fa, fB, fb = fAB + fAb, fab + faB, fAB + faB, fab + fAb
    linkD = fAB - fA * fB
    if fa == 0 or fA == 0 or fB == 0 or fb == 0:
        r2 = float("nan")
    else:
        r2 = linkD * linkD / (fA * fa * fB * fb)
    linkd = fab - fa * fb
    dp = float("nan")
    if linkd < 0:
        dp = linkd / max([-fA * fB, -fa * fb])
    elif linkD > 0:
        dp = linkd / min([fA * fb, fa * fB])
    return r2, dp


def replay_rows(AB, Ab, aB, ab):
    """ld_replay over the count columns of a table -> (r2[n], d_prime[n]) float64"""
    n = len(AB)
    r2, dp = np.empty(n, dtype=np.float64), np.empty(n, dtype=np.float64)
    for i, t in enumerate(zip(np.asarray(AB).tolist(), np.asarray(Ab).tolist(), np.asarray(aB).tolist(), np.asarray(ab).tolist())):
        r2[i], dp[i] = ld_replay(*t)
    return r2, dp


def same_bits(a, b):
    """NaN where the other is NaN, the same 64 bits everywhere else"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


def expected(w, lut, fb, **kw):
    """the oracle per split (oracle.profile_split on the split's own observations), tables concatenated; + n_edges / n_increments summed"""
    from oracle import oracle
    gpos = w["gpos"]
    pair = np.unique(w["pair"], return_inverse=True)[1].astype(np.int64)       # (the oracle takes int32 ids; relabelling changes no table)
    sb = w["split_bounds"]
    cut = np.searchsorted(gpos, sb)
    out = {"entries": [], "snv": [], "ld": []}
    n_edges = n_inc = 0
    for i in range(len(sb) - 1):
        a, e = int(cut[i]), int(cut[i + 1])
        if a == e:
            continue
        o = oracle.profile_split(gpos[a:e], w["base"][a:e], w["mm"][a:e], pair[a:e], "A" * int(sb[i + 1] - sb[i]), int(sb[i]), lut, fb, **kw)
        for k in out:
            out[k].append(o[k])
        n_edges += o["n_edges"]
        n_inc += o["n_increments"]
    dts = {"entries": oracle.ENTRY_DT, "snv": oracle.SNV_DT, "ld": oracle.LD_DT}
    res = {k: np.concatenate(v) if v else np.zeros(0, dtype=dts[k]) for k, v in out.items()}
    res["n_edges"], res["n_increments"] = n_edges, n_inc
    return res


# ---- the families' cases (shared by the CPU checks of the builder and the device tests) ------------------------------------------------

LADDER = [(1, 1), (2, 1), (2, 2), (15, 15), (16, 16), (16, 3), (17, 17), (17, 2), (63, 63), (64, 64), (64, 5), (65, 65), (65, 4), (128, 64),
          (128, 65), (200, 40), (300, 65), (511, 300), (512, 256), (513, 384), (1000, 767), (1000, 768), (5000, 100)]
FALLBACK = [(1000, 769), (2000, 900)]
REDUCED = [(1, 1), (2, 2), (16, 16), (17, 17), (32, 32), (33, 33), (64, 40), (65, 40), (512, 40), (513, 40)]


def ladder(M, plans=LADDER, extra=200, edge_first=0, **kw):
    """family A: plan i on first site i of a genome of len(plans) + extra sites (+ one site with `edge_first` unique keys on as many
    second sites: a single site that stages more than a flush's worth of edges)"""
    n = len(plans) + (1 if edge_first else 0)
    b = Builder(n + extra, **kw)
    for i, (ni, u) in enumerate(plans):
        b.plan(i, ni, u, M)
    if edge_first:
        b.plan(len(plans), edge_first, edge_first, M, edge_first=True)
    return b


def scan_firsts(K):
    f = [0, 1, 4093, 4094, 4095, 4096, 4097, K - 2] + ([8190, 8191] if K > 8192 else [])
    return sorted(set(k for k in f if 0 <= k <= K - 2))


def scan_case(K, every=False):
    """family B: K sites (bg 6 + 6); 25 two-site pairs k -> k + 1 for the first sites of scan_firsts(K) -- counts on the last element of
    a 4096-tile, the first of the next, in the scalar tail, behind two tiles' carry; every: three pairs k -> k + 1 for EVERY k instead"""
    b = Builder(K, 6, 6)
    if every:
        for k in range(K - 1):
            for b1, b2 in ((0, 0), (1, 1), (0, 1)):
                b.link([(k, b1), (k + 1, b2)])
    else:
        for k in scan_firsts(K):
            for i in range(25):
                b.link([(k, i & 1), (k + 1, (i >> 1) & 1)])
    return b


def long_pairs(independent=False):
    """family C: 200 pairs that each see all 40 sites, mm = i % 8 -> 156 000 increments on 780 edges, 6 240 rows (M = 8).  A pair carries one
    drawn base on every site (a haplotype: two combos an edge and level), the 25 pairs of level 0 a drawn base per site (four combos): site 0
    has 39 x (7 x 2 + 4) = 702 unique keys, within the bucket chain's 768.  independent: every base drawn by itself -- 39 x 8 x 4 = 1 248
    unique keys at site 0, so the batch grows its key table and THEN falls back to the sorted chain"""
    rng = np.random.default_rng(20261019)
    b = Builder(40)
    for i in range(200):
        bs = rng.integers(0, 2, 40)
        if not independent and i % 8:
            bs[:] = bs[0]
        b.link([(k, int(bs[k])) for k in range(40)], i % 8)
    return b


def self_pairs():
    """family C: three-site pairs; a pair twice on one column as (A, C) and another as (C, A) (the orientation is arrival order); a pair
    three times on one column; a pair twice on each of two sites"""
    rng = np.random.default_rng(7)
    b = Builder(10)
    for i in range(30):
        bs = rng.integers(0, 2, 3)
        b.link([(0, int(bs[0])), (1, int(bs[1])), (2, int(bs[2]))])
    for _ in range(3):
        b.link([(3, 0), (3, 1)])
        b.link([(3, 1), (3, 0)])
        b.link([(4, 0), (4, 0), (4, 1)])
        b.link([(5, 0), (5, 1), (6, 1), (6, 0)])
    for i in range(24):
        b.link([(7, i & 1), (8, (i >> 1) & 1)])
    return b


def pair_hash(ids, logH):
    return ((np.asarray(ids, dtype=np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - logH)


def hashed_case():
    """family C: self_pairs() + three pairs whose ids fall on one slot of the hashed heads (two interleave on the same two sites, the third
    sees one of them); ids above 2^20 + 8 * allele observations incl. 0 and 2^32 - 2 -> (builder, sparse id of every dense id, logH, the
    three dense ids)"""
    b = self_pairs()
    first_link = b.K * 60                                  # (the background pairs come first)
    p1 = b.link([(8, 0), (9, 1)])
    p2 = b.link([(8, 1), (9, 0)])
    p3 = b.link([(8, 1)])
    n_ao = len(b.pos)                                      # (every observation carries A or C at a called site)
    logH = 12
    while (1 << logH) < 2 * n_ao:
        logH += 1
    lo = (1 << 20) + 8 * n_ao + 1
    ids = lo + np.arange(b.n_pairs, dtype=np.uint64) * np.uint64(4099)
    ids[first_link], ids[first_link + 1] = 0, 2**32 - 2
    cand = np.arange(lo + 10_000_000, lo + 10_000_000 + (64 << logH), dtype=np.uint64)
    cand = cand[pair_hash(cand, logH) == pair_hash(cand[:1], logH)[0]][:3]
    assert len(cand) == 3
    ids[[p1, p2, p3]] = cand
    assert len(np.unique(ids)) == b.n_pairs
    return b, ids.astype(np.int64), logH, (p1, p2, p3)


def wave_case():
    """family C: columns whose LAST 64 observations (64 pairs, one a lane) have their pairs' earlier observation on 1, 2 and 64 distinct
    first sites; every column holds a multiple of 64 observations, so those 64 share a wave where a site's observations sit side by side"""
    K = 67
    n_link = [0] * K
    for k in range(64):
        n_link[k] = 1 + (64 if k == 0 else 32 if k in (1, 2) else 0)
    n_link[64] = n_link[65] = n_link[66] = 64
    b = Builder(K, bg=lambda k: (32, 32 + (-n_link[k]) % 64, 0, 0))
    for i in range(64):
        b.link([(0, i & 1), (64, (i >> 1) & 1)])
    for i in range(64):
        b.link([(1 + (i >= 32), i & 1), (65, (i >> 1) & 1)])
    for i in range(64):
        b.link([(i, i & 1), (66, (i >> 1) & 1)])
    return b


def split_bounds_for(b):
    """family D on the ladder genome: a bound between first site 4 and some of its second sites, one exactly on site 6, a split that is
    the single position of site 6, two empty splits behind it, a bound one past site 15"""
    p6 = site_pos(6)
    return [0, p6, p6 + 1, p6 + 2, p6 + 3, site_pos(15) + 1, site_pos(21) + 2, b.n_pos]


def many_splits_case(n_splits=2000):
    """family D: a short genome (2 100 sites, three pairs k -> k + 1 for every k) cut into n_splits splits of 3 or 4 positions"""
    b = scan_case(2100, every=True)
    sb = np.unique(np.linspace(0, b.n_pos, n_splits + 1).astype(np.int64))
    assert len(sb) == n_splits + 1
    return b, sb


def level_case(M):
    """family E: linking pairs at levels 0, M/2 - 1, M/2 and M - 1 (the key's mm field, site_cum over M levels); sites 8 / 9: site 8 holds
    level 5 only through pairs that reach site 10, not site 9"""
    b = Builder(12)
    for j, m in enumerate((0, M // 2 - 1, M // 2, M - 1)):
        for i in range(25):
            b.link([(2 * j, i & 1), (2 * j + 1, (i >> 1) & 1)], m)
            b.link([(0, (i >> 1) & 1), (11, i & 1)], m)
    for i in range(25):
        b.link([(8, i & 1), (9, (i >> 1) & 1)], 3)
        b.link([(8, (i >> 1) & 1), (10, i & 1)], 5)
    return b


def gate_case():
    """family F: pair tables of exactly 20 and 21 (the gate is strict); shallow columns whose two sites sum, linking observations
    included, to 19 (sites 4 + 5: 9 + 10) and 20 (sites 6 + 7) -- site_cum's sum on both sides of min_snp 20.  That gate can never decide
    a row by itself: every spanning pair adds an observation to both sites, so the sum is at least twice the pair table's total and the
    strict gate on the total (4 here) speaks first; the columns pin that such sites are called, linked and give no row.  Tied alleles
    (A = C; C = T without A; A = C = T = 32 at site 10: a third allele as deep as the two called ones) -- ties resolve A<C<T<G; a table
    with one allele absent among the spanning pairs (r2 and D' NaN)"""
    bg = {4: (3, 2, 0, 0), 5: (3, 3, 0, 0), 6: (3, 3, 0, 0), 7: (3, 3, 0, 0),
          9: (0, 25, 25, 0), 10: (20, 20, 32, 0), 11: (30, 30, 0, 0)}
    b = Builder(16, bg=lambda k: bg.get(k, (30, 30, 0, 0)))
    b.site_bases[9] = (1, 2)
    for i in range(20):
        b.link([(0, i & 1), (1, (i >> 1) & 1)])
    for i in range(21):
        b.link([(2, i & 1), (3, (i >> 1) & 1)])
    for i in range(4):
        b.link([(4, i & 1), (5, (i >> 1) & 1)])
        b.link([(6, i & 1), (7, (i >> 1) & 1)])
    for i in range(24):                                    # balanced: the ties stay ties
        b.link([(8, i & 1), (9, 1 + ((i >> 1) & 1)), (10, (i >> 2) & 1), (11, i & 1)])
    for i in range(30):                                    # every spanning pair carries A at site 12
        b.link([(12, 0), (13, i & 1)])
    for i in range(30):                                    # ... and C at site 15
        b.link([(14, i & 1), (15, 1)])
    return b


DENSE_SPLIT_SITES = [1, 2, 7, 8, 9, 31, 32, 33, 129, 2, 2, 2]


def dense_tile_case():
    """family G: splits of 1, 2, 7, 8, 9, 31, 32, 33 and 129 sites (ctiles = ceil(4 sites / 32), blocks of four column tiles), then three
    two-site splits with 127, 128 and 129 distinct pairs (rows padded to 128); one pair twice on a column with the same base"""
    K = sum(DENSE_SPLIT_SITES)
    b = Builder(K)
    first, bounds = 0, [0]
    for j, n in enumerate(DENSE_SPLIT_SITES):
        for k in range(first, first + n - 1):
            for b1, b2 in ((0, 0), (1, 1), (0, 1)):
                b.link([(k, b1), (k + 1, b2)])
            if k + 5 < first + n:
                b.link([(k, 1), (k + 5, 0)])
                b.link([(k, 0), (k + 3, 0), (k + 5, 1)])
        if j >= 9:                                         # 120 background pairs + 3 above + these = 127 / 128 / 129 rows
            for i in range(j - 9 + 4):
                b.link([(first, i & 1), (first + 1, 1)])
            if j == 9:
                b.pos.append(site_pos(first)); b.base.append(1); b.mm.append(0); b.pair.append(b.n_pairs - 1)     # X cell = 2
        first += n
        bounds.append(site_pos(first) - 1 if first < K else b.n_pos)
    return b, bounds
