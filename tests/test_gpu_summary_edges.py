"""GPU: the per-scaffold summary (isx_summary.hip run_summary: k_level_dense / k_patch_saturated / k_level_apply / k_seg_reduce /
k_pick_median / the rocPRIM sorts / k_pack_rows, behind Batch.summarize and Slot.summarize) at its tile, sort, median, presence and
saturation edges, against tests/summary_ref.py -- plain numpy in float64 on the observations, pinned on the host by
tests/test_summary_ref.py.  Expected coverage is np.bincount of the observations, expected clonalities come from the CPU oracle scaffold
by scaffold.  Nothing expected is read back from the device, with one exception: the rarefied clonalities are random in the reference,
so their per-(position, mm) values are the product's own (fetch / collect) and only what the summary makes of them is checked.

Integers and medians must be equal (a median of float32 values is exact in float64).  sum_clon / sum_clon_rarefied are float64 atomic
sums in arbitrary order: |got - fsum| <= (n - 1) * 2**-53 * fsum + one ulp, n = counted (summary_ref.sum_bound)."""
import functools

import numpy as np
import pytest

from instrain_amd import _lib, engine
from tests import summary_ref as sr, util
from tests.test_gpu_rollup_edges import _reads

pytestmark = pytest.mark.gpu
INT_FIELDS = ("nonzero", "sum_cov", "sumsq_cov", "counted", "counted_rarefied")
MEDIANS = ("median_cov", "median_clon", "median_clon_rarefied")
SUMS = (("sum_clon", "counted"), ("sum_clon_rarefied", "counted_rarefied"))
RARE = 6                        # rarefied_coverage of most cases: low enough for some positions of a depth-5 input to have a value
LETTERS = np.array(list("ACTG"))


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    lut, fb = util.load_lut()
    c.set_null_model(lut, fb)
    yield c
    c.close()


# ---- plumbing ----
def _sorted(gpos, base, mm, pair):
    o = np.argsort(gpos, kind="stable")
    return gpos[o].astype(np.int64), base[o].astype(np.uint8), mm[o].astype(np.int64), pair[o].astype(np.uint32)


def _bases(rng, gpos, codes, keep=0.85):
    return np.where(rng.random(len(gpos)) < keep, codes[gpos], rng.integers(0, 4, len(gpos))).astype(np.uint8)


def _batch(ctx, codes, split_bounds, gpos, base, mm, pair, M, rare=RARE):
    b = engine.Batch(ctx, codes, split_bounds, engine.pack_obs(gpos.astype(np.uint32), base, mm), pair, n_mm_bins=M, enable_linkage=False,
                     rarefied_coverage=rare)
    b.run()
    return b


def _pipe_slot(ctx, codes, split_bounds, gpos, base, mm, pair, M, rare=RARE, want_counts=None):
    """the observations through a read-level pipe -> (pipe, ticket, collect()'s dict)"""
    segs = util.reassemble_segs(gpos.astype(np.uint32), base, mm, pair)
    pipe = engine.Pipe(ctx, max_pos=len(codes), max_obs=0, max_segs=segs.n_seg, max_splits=len(split_bounds), depth=1, host_threads=2,
                       n_mm_bins=M, enable_linkage=False, rarefied_coverage=rare, want_counts=(M == 1) if want_counts is None else want_counts,
                       layout=_lib.LAYOUT_MM_ENTRIES if M > 1 else 0)
    t = pipe.submit_reads(codes, split_bounds, segs)
    return pipe, t, pipe.collect(t)


def _own_rarefied(res, n_pos, M):
    """THE EXCEPTION: the product's own rarefied clonalities (random in the reference) laid out per level like the others"""
    if M > 1:
        e = res["entries"]
        return sr.entry_levels(e["gpos"], e["mm"], e["clon_rarefied"], n_pos, M)
    if "clon_r" in res:
        return np.asarray(res["clon_r"], dtype=np.float64)[None].copy()
    out = np.full((1, n_pos), np.nan)
    out[0, res["rare"]["gpos"]] = res["rare"]["clon_rarefied"]
    return out


def _assert_rows(rows, exp, what):
    """element by element: integers and medians equal, present equal, the two float sums inside the bound of their operation"""
    assert rows.shape == exp["nonzero"].shape and (rows["mm"] == np.arange(rows.shape[1])[None, :]).all(), what
    for f in INT_FIELDS:
        assert (rows[f].astype(np.int64) == exp[f]).all(), (what, f, np.argwhere(rows[f].astype(np.int64) != exp[f])[:5])
    assert ((rows["present"] != 0) == exp["present"]).all(), (what, "present", np.argwhere((rows["present"] != 0) != exp["present"])[:5])
    for f in MEDIANS:
        bad = ~((rows[f] == exp[f]) | (np.isnan(rows[f]) & np.isnan(exp[f])))
        assert not bad.any(), (what, f, np.argwhere(bad)[:5], rows[f][bad][:5], exp[f][bad][:5])
    for f, cnt in SUMS:
        for i, m in np.ndindex(rows.shape):
            # n terms added in some order against math.fsum of them: (n - 1) * 2**-53 * fsum + one ulp (summary_ref.sum_bound)
            tol = sr.sum_bound(exp[cnt][i, m], exp[f][i, m])
            assert abs(float(rows[f][i, m]) - exp[f][i, m]) <= tol, (what, f, i, m, float(rows[f][i, m]), exp[f][i, m], tol)


def _same_but_sums(a, b):
    return all(a[f].tobytes() == b[f].tobytes() for f in a.dtype.names if f not in ("sum_clon", "sum_clon_rarefied"))


def _summarize_twice(obj, bounds, what):
    rows, ms = obj.summarize(bounds)
    again, _ = obj.summarize(bounds)
    assert ms > 0 and _same_but_sums(rows, again), what
    return rows


def _expected(bounds, gpos, base, mm, pair, seq, M, clon_r, vectorised=False):
    n_pos = int(bounds[-1])
    cov = sr.cov_levels(gpos, base, mm, n_pos, M)
    if vectorised:
        clon = sr.clon_levels_from_counts(gpos, base, mm, n_pos, M)
    else:
        lut, fb = util.load_lut()
        clon, _ = sr.oracle_levels(bounds, gpos, base, mm, pair, seq, M, lut, fb)
    return sr.scaffold_levels(cov, clon, clon_r, sr.presence(gpos, base, mm, bounds, M), bounds), cov, clon


# ---- a. tile and scaffold edges ----
def _tile_layout(edge16k, whole):
    """(start, end, has reads).  edge16k 'on': one scaffold ends exactly on 16 384 and the next starts there; 'across': one scaffold runs
    from below 16 384 to above it (the two cannot hold at once)"""
    lay = [(0, 63, False), (63, 64, True), (64, 65, True), (65, 127, True), (127, 128, True), (128, 129, True),
           (129, 130, True), (130, 132, True), (132, 135, True), (135, 136, True), (136, 137, True),        # 1, 2, 3, 1, 1 inside tile 2
           (137, 1000, True), (1000, 5000, False), (5000, 12000, True)]
    lay += [(12000, 16384, True), (16384, 16500, True)] if edge16k == "on" else [(12000, 16500, True)]
    lay += [(16500, 20000, True), (20000, 32000, True), (32000, 2 * sr.BLOCK + (0 if whole else 1), False)]
    return lay


@functools.lru_cache(maxsize=None)
def _tile_case(M, edge16k, whole):
    lay = _tile_layout(edge16k, whole)
    bounds = np.array([s for s, _, _ in lay] + [lay[-1][1]], dtype=np.int64)
    n_pos = int(bounds[-1])
    # the layout really has the edges it is here for
    assert all(a[1] == b[0] for a, b in zip(lay, lay[1:])) and n_pos == 2 * sr.BLOCK + (0 if whole else 1)
    assert (n_pos % sr.TILE != 0) == (not whole) and (n_pos % sr.BLOCK == 0) == whole
    assert {63, 64, 65, 127, 128, 129} <= set(bounds.tolist())
    run = [i for i in range(len(lay) - 4) if [e - s for s, e, _ in lay[i:i + 5]] == [1, 2, 3, 1, 1]]
    assert len(run) == 1 and lay[run[0]][0] // sr.TILE == (lay[run[0] + 4][1] - 1) // sr.TILE
    if edge16k == "on":
        assert sr.BLOCK in bounds.tolist() and all(r for s, e, r in lay if e == sr.BLOCK or s == sr.BLOCK)
    else:
        assert any(s < sr.BLOCK < e and r for s, e, r in lay) and sr.BLOCK not in bounds.tolist()
    empty = [i for i, (_, _, r) in enumerate(lay) if not r]
    assert empty[0] == 0 and empty[-1] == len(lay) - 1 and len(empty) == 3
    rng = np.random.Generator(np.random.PCG64(4100 + 10 * M + (edge16k == "on") + 2 * whole))
    gpos, mm, pair = _reads(rng, bounds, 5, M, skip=empty)
    codes = rng.integers(0, 4, n_pos).astype(np.uint8)
    base = _bases(rng, gpos, codes)
    return bounds, gpos, base, mm, pair, codes, "".join(LETTERS[codes]), empty


@pytest.mark.parametrize("whole", [False, True])
@pytest.mark.parametrize("edge16k", ["on", "across"])
@pytest.mark.parametrize("M", [1, 3])
def test_summary_tile_and_scaffold_edges_batch(ctx, M, edge16k, whole):
    """k_seg_reduce's tile walk (64 positions a lane, 16 384 a workgroup) through Batch.summarize, dense arrays (M = 1) and entries
    (M = 3): scaffold ends on 63, 64, 65, 127, 128 and 129 (a bound on a multiple of 64 and one position to either side); scaffolds of
    1, 2, 3, 1 and 1 positions inside one tile (flush after flush in one lane); a scaffold that crosses 16 384 ('across') or one that
    ends exactly there and one that starts there ('on'); the first, a middle and the last scaffold without a read; n_pos = 2 * 16 384 + 1
    (no multiple of 64: one lane of a third workgroup holds one position) and 2 * 16 384 (the last workgroup is full, no spare lane).
    Every field of every (scaffold, level) against summary_ref; two calls give the same bytes except the float sums."""
    bounds, gpos, base, mm, pair, codes, seq, empty = _tile_case(M, edge16k, whole)
    b = _batch(ctx, codes, bounds, gpos, base, mm, pair, M)
    rows = _summarize_twice(b, bounds, (M, edge16k, whole))
    clon_r = _own_rarefied(b.fetch(), int(bounds[-1]), M)
    b.close()
    exp, cov, _ = _expected(bounds, gpos, base, mm, pair, seq, M, clon_r)
    _assert_rows(rows, exp, (M, edge16k, whole))
    assert not exp["present"][empty].any() and not exp["sum_cov"][empty].any() and np.isnan(rows["median_clon"][empty]).all()
    assert (rows["median_cov"][empty] == 0).all() and exp["counted"][:, -1].sum() > 10000 and exp["counted_rarefied"][:, -1].sum() > 1000
    assert (exp["nonzero"][6:11, -1] == [1, 2, 3, 1, 1]).all()              # the run inside one tile: every one of them covered throughout


@pytest.mark.parametrize("M", [1, 3])
def test_summary_tile_and_scaffold_edges_slot(ctx, M):
    """the same layout ('on', n_pos = 2 * 16 384 + 1) through Slot.summarize of a read-level pipe: with the count table at M = 1, the
    entries layout at M = 3"""
    bounds, gpos, base, mm, pair, codes, seq, _ = _tile_case(M, "on", False)
    pipe, t, res = _pipe_slot(ctx, codes, bounds, gpos, base, mm, pair, M)
    rows = _summarize_twice(res["slot"], bounds, ("slot", M))
    clon_r = _own_rarefied(res, int(bounds[-1]), M)
    pipe.release(t)
    pipe.close()
    exp, _, _ = _expected(bounds, gpos, base, mm, pair, seq, M, clon_r)
    _assert_rows(rows, exp, ("slot", M))


# ---- b. the median pick ----
def _pile(rng, piles, M):
    """piles: {flat position: (A, C, T, G) counts} -> single-position reads, each its own pair, with random levels"""
    gpos = np.concatenate([np.full(sum(c), p, dtype=np.int64) for p, c in piles.items()])
    base = np.concatenate([np.repeat(np.arange(4, dtype=np.uint8), c) for c in piles.values()])
    return _sorted(gpos, base, rng.integers(0, M, len(gpos)), np.arange(len(gpos), dtype=np.uint32))


MIXES = [(5, 1, 0, 0), (3, 3, 0, 0), (6, 0, 2, 1), (2, 2, 2, 2), (7, 0, 0, 1)]     # five positions at min_cov or above, five distinct clonalities


@pytest.mark.parametrize("M", [1, 2])
def test_summary_median_pick(ctx, M):
    """k_pick_median on hand-built scaffolds: length 1 (n = 1); length 2 with coverages (0, 7) -> 3.5 (n = 2, the middle two differ);
    length 5 (odd) and 6 (even, middle values 3 and 5 -> 4.0); three scaffolds of about 300 positions where only 1, 2 and 5 positions
    reach min_cov with distinct clonalities, so that `counted` (not the segment length) must pick the median -- the first `counted` of
    the sorted values, NaN behind them; and one with counted == 0 -> NaN.  With two levels the same piles are spread over the levels."""
    rng = np.random.Generator(np.random.PCG64(50 + M))
    lens = [1, 2, 5, 6, 300, 301, 299, 300]
    bounds = np.r_[0, np.cumsum(lens)].astype(np.int64)
    n_pos = int(bounds[-1])
    codes = np.zeros(n_pos, dtype=np.uint8)
    piles = {0: (7, 0, 0, 0), 2: (7, 0, 0, 0)}
    piles.update({int(bounds[2]) + i: (c, 0, 0, 0) for i, c in enumerate([1, 2, 9, 4, 6])})
    piles.update({int(bounds[3]) + i: (c, 0, 0, 0) for i, c in enumerate([3, 1, 8, 5, 2, 9])})
    for s in (4, 5, 6, 7):                                               # a background below min_cov, some positions bare
        piles.update({int(p): (int(rng.integers(1, 5)), 0, 0, 0) for p in range(int(bounds[s]), int(bounds[s + 1])) if rng.random() < 0.8})
    for s, k in ((4, 1), (5, 2), (6, 5)):
        for p, c in zip(rng.choice(np.arange(int(bounds[s]), int(bounds[s + 1])), k, replace=False), MIXES):
            piles[int(p)] = c
    gpos, base, mm, pair = _pile(rng, piles, M)
    b = _batch(ctx, codes, bounds, gpos, base, mm, pair, M)
    rows = _summarize_twice(b, bounds, M)
    clon_r = _own_rarefied(b.fetch(), n_pos, M)
    b.close()
    exp, cov, clon = _expected(bounds, gpos, base, mm, pair, "".join(LETTERS[codes]), M, clon_r)
    _assert_rows(rows, exp, M)
    # the answers known by hand, at the last level (all observations)
    assert rows["median_cov"][:4, -1].tolist() == [7.0, 3.5, 4.0, 4.0] and rows["counted"][:, -1].tolist() == [1, 1, 2, 3, 1, 2, 5, 0]
    c = sr.clonality(np.array(MIXES))
    assert len(set(c.tolist())) == 5
    assert rows["median_clon"][4:, -1].tolist()[:3] == [c[0], (c[0] + c[1]) / 2, float(np.median(c))] and np.isnan(rows["median_clon"][7]).all()
    assert c[0] != c[1] and rows["median_clon"][2, -1] == 1.0 and rows["median_clon"][3, -1] == 1.0


# ---- c. level presence ----
@functools.lru_cache(maxsize=None)
def _presence_case():
    bounds = np.array([0, 300, 599, 900, 1200], dtype=np.int64)
    rng = np.random.Generator(np.random.PCG64(333))
    gpos, mm, pair = _reads(rng, bounds, 6, 4, skip=(3,))
    sc = np.searchsorted(bounds, gpos, side="right") - 1
    lv1, lv2 = rng.choice([0, 3], int(pair.max()) + 1), rng.choice([0, 1, 3], int(pair.max()) + 1)
    mm = np.where(sc == 1, lv1[pair], np.where(sc == 2, lv2[pair], mm))           # one level per read, redrawn for scaffolds 1 and 2
    codes = rng.integers(0, 4, 1200).astype(np.uint8)
    base = _bases(rng, gpos, codes)
    # the only level-2 read of scaffold 2: 25 positions of base code 4 (N)
    n_at = np.arange(700, 725, dtype=np.int64)
    gpos, base = np.r_[gpos, n_at], np.r_[base, np.full(25, 4, dtype=np.uint8)]
    mm, pair = np.r_[mm, np.full(25, 2)], np.r_[pair, np.full(25, int(pair.max()) + 1)]
    gpos, base, mm, pair = _sorted(gpos, base, mm, pair)
    return bounds, gpos, base, mm, pair, codes, "".join(LETTERS[codes])


@pytest.mark.parametrize("M", [4, 1])
def test_summary_level_presence(ctx, M):
    """four scaffolds of about 300 positions: reads at every level; levels 0 and 3 only (coverage carries over levels 1 and 2, present
    0 there); a level 2 that exists only through one read showing base code 4 (N) throughout (count sum 0, yet the level is present:
    the rule in k_level_apply's comment); no read at all.  The same observations at M = 1 (dense path), where present = any coverage."""
    bounds, gpos, base, mm, pair, codes, seq = _presence_case()
    if M == 1:
        mm = np.zeros_like(mm)
    sc = np.searchsorted(bounds, gpos, side="right") - 1
    assert (base[(sc == 2) & (mm == 2)] == 4).all() and ((sc == 2) & (mm == 2)).sum() == (25 if M == 4 else 0) and not (sc == 3).any()
    b = _batch(ctx, codes, bounds, gpos, base, mm, pair, M)
    rows = _summarize_twice(b, bounds, M)
    clon_r = _own_rarefied(b.fetch(), 1200, M)
    b.close()
    exp, cov, _ = _expected(bounds, gpos, base, mm, pair, seq, M, clon_r)
    _assert_rows(rows, exp, M)
    if M == 4:
        assert (rows["present"] != 0).tolist() == [[True] * 4, [True, False, False, True], [True] * 4, [False] * 4]
        for f in INT_FIELDS + MEDIANS:                                   # carried over the absent levels, and over the N-only level
            assert rows[f][1, 1].tobytes() == rows[f][1, 0].tobytes() == rows[f][1, 2].tobytes(), f
            if "rarefied" not in f:                                      # (the N-only entries draw rarefied values of their own)
                assert rows[f][2, 2].tobytes() == rows[f][2, 1].tobytes(), f
        assert rows["sum_cov"][1, 3] > rows["sum_cov"][1, 0] > 0 and rows["sum_cov"][2, 3] > rows["sum_cov"][2, 2]
    else:
        assert (rows["present"][:, 0] != 0).tolist() == [True, True, True, False]
    assert rows["sum_cov"][:, -1].tolist() == [int(((sc == i) & (base < 4)).sum()) for i in range(4)]


# ---- d. the sort split ----
@pytest.mark.parametrize("lens", [(sr.BIG_SEG, sr.BIG_SEG + 1, 300, sr.BIG_SEG + 1), (sr.BIG_SEG + 1, sr.BIG_SEG + 1)])
@pytest.mark.parametrize("M", [1, 2])
def test_summary_sort_split(ctx, M, lens):
    """run_summary sorts segments above BIG_SEG = 131 072 one by one with the device-wide radix sort and hands them to the segmented
    sort as empty ranges: 131 072 (the small path's largest), 131 073 (big), 300 (small), 131 073 (big) in this order; and two of
    131 073 alone, where no segment is small and the segmented sort is skipped.  Expected clonalities vectorised from the base counts
    (summary_ref.clon_levels_from_counts), cross-checked here against the CPU oracle on the 300-position scaffold."""
    bounds = np.r_[0, np.cumsum(lens)].astype(np.int64)
    n_pos = int(bounds[-1])
    small = [ln <= sr.BIG_SEG for ln in lens]
    assert any(small) == (len(lens) == 4) and (len(lens) == 2 or (lens[0] == 1 << 17 and small == [True, False, True, False]))
    rng = np.random.Generator(np.random.PCG64(1700 + M + len(lens)))
    gpos, mm, pair = _reads(rng, bounds, 3, M)
    codes = rng.integers(0, 4, n_pos).astype(np.uint8)
    base = _bases(rng, gpos, codes)
    b = _batch(ctx, codes, bounds, gpos, base, mm, pair, M)
    rows = _summarize_twice(b, bounds, (M, lens))
    clon_r = _own_rarefied(b.fetch(), n_pos, M)
    b.close()
    exp, cov, clon = _expected(bounds, gpos, base, mm, pair, None, M, clon_r, vectorised=True)
    if len(lens) == 4:
        lut, fb = util.load_lut()
        s0, s1 = int(bounds[2]), int(bounds[3])
        k = (gpos >= s0) & (gpos < s1)
        o, _ = sr.oracle_levels([0, 300], gpos[k] - s0, base[k], mm[k], pair[k], "".join(LETTERS[codes[s0:s1]]), M, lut, fb)
        assert np.array_equal(o, clon[:, s0:s1], equal_nan=True) and (~np.isnan(o[-1])).sum() > 10
    _assert_rows(rows, exp, (M, lens))
    assert (exp["counted"][:, -1] > 0).all() and (exp["counted"][:, -1] < np.array(lens) // 2).all()    # counted far below the segment length


# ---- e. saturated coverage on a slot without a count table ----
def test_summary_saturated_slot_without_counts(ctx):
    """a pipe slot created without want_counts keeps 16-bit saturating coverage and the list of saturated positions; k_patch_saturated
    patches a position only when its listed value is >= 65 535.  One split cut into three scaffolds by the bounds, a background of
    depth 3 and four spots of single-position reads with coverage exactly 65 534 and 65 535 (both in the first tile of the second
    scaffold), 65 536 (on that scaffold's last position) and 70 001: sum_cov, sumsq_cov (far from what 16 bits would give), nonzero
    and median_cov against np.bincount in Python integers; a Batch of the same observations (which has the count table) gives the
    same rows."""
    bounds = np.array([0, 1000, 2000, 3000], dtype=np.int64)
    rng = np.random.Generator(np.random.PCG64(65535))
    gpos, mm, pair = _reads(rng, np.array([0, 3000]), 3, 1)
    spots = {1003: 65534, 1010: 65535, 1999: 65536, 2500: 70001}
    bg = np.bincount(gpos, minlength=3000)
    extra = np.concatenate([np.full(d - bg[p], p, dtype=np.int64) for p, d in spots.items()])
    pair = np.r_[pair, int(pair.max()) + 1 + np.arange(len(extra))]
    gpos = np.r_[gpos, extra]
    codes = rng.integers(0, 4, 3000).astype(np.uint8)
    base = _bases(rng, gpos, codes, keep=0.7)
    gpos, base, mm, pair = _sorted(gpos, base, np.zeros(len(gpos), dtype=np.int64), pair)
    cov = sr.cov_levels(gpos, base, mm, 3000, 1)
    assert [int(cov[0, p]) for p in spots] == list(spots.values()) and np.delete(cov[0], list(spots)).max() < 50
    assert 1003 // sr.TILE == 1010 // sr.TILE == 1000 // sr.TILE and 1999 == bounds[2] - 1
    clon = sr.clon_levels_from_counts(gpos, base, mm, 3000, 1)
    present = sr.presence(gpos, base, mm, bounds, 1)
    got = {}
    for how in ("slot", "batch"):
        if how == "slot":
            pipe, t, res = _pipe_slot(ctx, codes, np.array([0, 3000]), gpos, base, mm, pair, 1, rare=50, want_counts=False)
            assert "counts" not in res and res["n_saturated"] >= 3
            rows = _summarize_twice(res["slot"], bounds, how)
            clon_r = _own_rarefied(res, 3000, 1)
            pipe.release(t)
            pipe.close()
        else:
            b = _batch(ctx, codes, np.array([0, 3000]), gpos, base, mm, pair, 1, rare=50)
            rows = _summarize_twice(b, bounds, how)
            clon_r = _own_rarefied(b.fetch(), 3000, 1)
            b.close()
        exp = sr.scaffold_levels(cov, clon, clon_r, present, bounds)
        _assert_rows(rows, exp, how)
        for i in range(3):                                              # the four named fields once more, in Python integers
            c = [int(x) for x in cov[0, int(bounds[i]):int(bounds[i + 1])]]
            assert (int(rows["sum_cov"][i, 0]), int(rows["sumsq_cov"][i, 0]), int(rows["nonzero"][i, 0])) == \
                (sum(c), sum(x * x for x in c), sum(1 for x in c if x)), (how, i)
            assert float(rows["median_cov"][i, 0]) == float(np.median(c))
        got[how] = rows
    assert int(got["slot"]["sumsq_cov"][1, 0]) > 65534 ** 2 + 65535 ** 2 + 65536 ** 2
    for f in INT_FIELDS[:4] + MEDIANS[:2] + ("present",):
        assert got["slot"][f].tobytes() == got["batch"][f].tobytes(), f
