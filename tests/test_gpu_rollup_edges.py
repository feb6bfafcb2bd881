"""GPU: the gene and genome roll-up kernels (isx_genes.hip k_gene_cov / k_scaffold_any / the SNV half, isx_genomes.hip k_genome_hist /
k_snv_levels / k_ld_levels) at their tile, stride and scaffold edges, against plain numpy / pandas restatements (tests/genome_ref.py,
tests/gene_ref.py) and the pinned oracle.  Expected coverage is np.bincount of the observations, so a pileup error cannot hide a roll-up
error or the other way round.  Every input comes from a seeded numpy Generator."""
import math

import numpy as np
import pandas as pd
import pytest

from instrain_amd import _lib, engine
from instrain_amd.profile import gene_profile
from tests import gene_ref, genome_ref, util
from tests.test_genes_host import keyed_types
from tests.test_gpu_genes import assert_counts_equal
from tests.test_gpu_genome_info import _median

pytestmark = pytest.mark.gpu
TILE = 4096                     # positions per workgroup of k_genome_hist, per wave of k_scaffold_any
MASK = 100
ACC_FIELDS = ("n", "sum_cov", "sumsq_cov", "max_cov")


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    lut, fb = util.load_lut()
    c.set_null_model(lut, fb)
    yield c
    c.close()


# ---- observations as reads: every read lies inside one scaffold, has one mm level and is its own pair ----
def _reads(rng, bounds, depth, M, read_len=25, skip=()):
    """-> (gpos, mm, pair) of the observations in gpos order: about `depth` reads over every position of every scaffold not in `skip`"""
    starts, lens = [], []
    for s in range(len(bounds) - 1):
        ln = int(bounds[s + 1] - bounds[s])
        if s in skip:
            continue
        L = min(read_len, ln)
        n = max(1, int(round(depth * ln / L)))
        starts.append(int(bounds[s]) + rng.integers(0, ln - L + 1, n))
        lens.append(np.full(n, L, dtype=np.int64))
    starts, lens = np.concatenate(starts), np.concatenate(lens)
    rid = np.repeat(np.arange(len(starts)), lens)
    gpos = starts[rid] + (np.arange(len(rid)) - np.repeat(np.cumsum(lens) - lens, lens))
    mm = rng.integers(0, M, len(starts))[rid]
    o = np.argsort(gpos, kind="stable")
    return gpos[o].astype(np.int64), mm[o].astype(np.int64), rid[o].astype(np.uint32)


def _cov_levels(gpos, mm, n_pos, M):
    """[M, n_pos]: the cumulative coverage of every position at every level, from the observations alone"""
    return np.stack([np.bincount(gpos[mm <= j], minlength=n_pos) for j in range(M)]).astype(np.int64)


def _batch(ctx, ref, bounds, gpos, base, mm, M, pair=None):
    b = engine.Batch(ctx, ref, bounds, engine.pack_obs(gpos.astype(np.uint32), base, mm), pair, n_mm_bins=M, enable_linkage=False)
    b.run()
    return b


def _slot(ctx, ref, bounds, gpos, base, mm, pair, M):
    """the same observations through a read-level pipe (M == 1: dense arrays, else the entries layout) -> (pipe, ticket, slot)"""
    segs = util.reassemble_segs(gpos.astype(np.uint32), base, mm, pair)
    pipe = engine.Pipe(ctx, max_pos=len(ref), max_obs=0, max_segs=segs.n_seg, max_splits=len(bounds), depth=1, host_threads=2, n_mm_bins=M,
                       enable_linkage=False, want_counts=M == 1, layout=_lib.LAYOUT_MM_ENTRIES if M > 1 else 0)
    t = pipe.submit_reads(ref, bounds, segs)
    return pipe, t, pipe.collect(t)["slot"]


def _assert_cov_equal(acc, hist, exp_acc, exp_hist, what):
    assert hist.shape == exp_hist.shape, (what, hist.shape, exp_hist.shape)
    for f in ACC_FIELDS:
        assert (acc[f] == exp_acc[f]).all(), (what, f, acc[f], exp_acc[f])
    assert (hist == exp_hist).all(), (what, np.argwhere(hist != exp_hist)[:5])


# ---- a. the genome histogram at tile and mask edges ----
# (start, end, genome) with MASK = 100; genome 3 is used by no scaffold.  28 673 positions: seven full tiles and one position.
EDGE_LAYOUT = [
    (0, 199, 0), (199, 399, 0), (399, 600, 0),                      # 2 * mask - 1, 2 * mask, 2 * mask + 1 in a row
    (600, 1000, 0), (1000, 1400, 1), (1400, 1800, 0), (1800, 2200, -1), (2200, 2600, 0), (2600, 3000, 2),      # tile 0: 0, 1, 0, -1, 0, 2
    (3000, 3996, 2),
    (3996, 6000, 1),                                                # interior begins exactly at 4096
    (6000, 8292, 4),                                                # interior ends exactly at 8192
    (8292, 12189, 0),
    (12189, 22190, 2),                                              # starts 99 before the tile edge 12288 (that tile counts nothing of it), interior
                                                                    # begins at 12289, spans tiles 3, 4 and 5; 10 001 long: one position at mask 5000
    (22190, 24576, 1),                                              # ends on a tile edge
    (24576, 26000, -1), (26000, 28672, -1),                         # tile 6: scaffolds of no genome only
    (28672, 28673, 4),                                              # the last tile holds one position
]
N_GENOMES = 5


def _edge_case(M, whole_tiles):
    lay = EDGE_LAYOUT[:-1] if whole_tiles else EDGE_LAYOUT
    bounds = np.array([s for s, _, _ in lay] + [lay[-1][1]], dtype=np.int64)
    genome = [g for _, _, g in lay]
    assert all(a[1] == b[0] for a, b in zip(lay, lay[1:])) and (int(bounds[-1]) % TILE == 0) == whole_tiles
    rng = np.random.Generator(np.random.PCG64(2024 + M))
    gpos, mm, pair = _reads(rng, bounds, 3, M)
    base = rng.integers(0, 4, len(gpos)).astype(np.uint8)
    ref = rng.integers(0, 4, int(bounds[-1])).astype(np.uint8)
    return bounds, genome, gpos, base, mm, pair, ref


@pytest.mark.parametrize("whole_tiles", [False, True])
@pytest.mark.parametrize("M", [1, 3])
def test_genome_hist_tile_and_mask_edges(ctx, M, whole_tiles):
    """k_genome_hist on a layout that puts a masked interior's begin on 4096, an end on 8192, a begin one past a tile edge, a scaffold
    start inside the mask before a tile edge, a scaffold over three tiles, lengths 199 / 200 / 201, one tile with genomes 0, 1, 0, -1, 0,
    2 (flush, accumulate again, flush again), a tile of no genome, a genome without scaffolds and a last tile of one position (or none:
    whole_tiles); mask_edges 0, 1, 100 and 5000 (one position of the 10 001 long scaffold counts).  Dense arrays (M = 1) and the entries
    layout (M = 3).  acc and hist equal the numpy reference element for element; a second call returns the same bytes."""
    bounds, genome, gpos, base, mm, _, ref = _edge_case(M, whole_tiles)
    cov = _cov_levels(gpos, mm, int(bounds[-1]), M)
    assert int(cov[-1].max()) < 64
    b = _batch(ctx, ref, bounds, gpos, base, mm, M)
    for mask in (0, 1, 100, 5000):
        exp_acc, exp_hist = genome_ref.coverage_rows_flat(cov, bounds, genome, N_GENOMES, mask_edges=mask, hist_bins=64)
        acc, hist, _ = b.genome_coverage_raw(bounds, genome, N_GENOMES, mask_edges=mask, hist_bins=64)
        _assert_cov_equal(acc, hist, exp_acc, exp_hist, (M, mask))
        acc2, hist2, _ = b.genome_coverage_raw(bounds, genome, N_GENOMES, mask_edges=mask, hist_bins=64)
        assert acc.tobytes() == acc2.tobytes() and hist.tobytes() == hist2.tobytes(), mask
        assert not hist[3].any() and not any(acc[f][3].any() for f in ACC_FIELDS)
        if mask == 5000:
            assert (acc["n"][2] == 1).all() and acc["n"].sum() == M
        if mask == 100:
            # 199 and 200 count nothing, 201 one position; the scaffolds of genome 0 add up
            assert acc["n"][0, 0] == 1 + 3 * 200 + (12189 - 8292 - 200)
    b.close()


# ---- b. both histogram paths, and depth beyond the LDS histogram ----
def test_genome_hist_lds_and_global_paths_deep(ctx):
    """six positions 8192 .. 9500 deep over two genomes, four inside masked interiors and two inside masked edges (not counted), on a
    background of ~5: hist_bins 2, 8191, 8192 (the LDS path's last size), 8193 and 16384 (global atomics) all give the reference's acc and
    bincount(min(c, bins - 1)); the two paths agree bin for bin; genome_coverage(hist_bins=4096) repeats into 16 384 exact bins"""
    bounds = np.array([0, 1500, 3300, 4500, 6000], dtype=np.int64)
    genome = [0, 1, 0, 1]
    rng = np.random.Generator(np.random.PCG64(77))
    gpos, mm, _ = _reads(rng, bounds, 5, 1)
    deep = {700: 8192, 1450: 9450, 2000: 8193, 3250: 9400, 4000: 9000, 4600: 9100}      # 1450 and 3250: inside masked edges, the deepest
    gpos = np.sort(np.concatenate([gpos] + [np.full(d, p, dtype=np.int64) for p, d in deep.items()]))
    mm = np.zeros(len(gpos), dtype=np.int64)
    base = rng.integers(0, 4, len(gpos)).astype(np.uint8)
    cov = _cov_levels(gpos, mm, 6000, 1)
    assert all(8192 <= cov[0, p] <= 9500 for p in deep) and cov[0, 1450] > cov[0, 4600] > cov[0, 4000]
    b = _batch(ctx, rng.integers(0, 4, 6000).astype(np.uint8), bounds, gpos, base, mm, 1)
    got = {}
    for bins in (2, 8191, 8192, 8193, 16384):
        exp_acc, exp_hist = genome_ref.coverage_rows_flat(cov, bounds, genome, 2, mask_edges=MASK, hist_bins=bins)
        acc, hist, _ = b.genome_coverage_raw(bounds, genome, 2, mask_edges=MASK, hist_bins=bins)
        _assert_cov_equal(acc, hist, exp_acc, exp_hist, bins)
        got[bins] = hist
    assert (acc["max_cov"][:, 0] == [cov[0, 4000], cov[0, 4600]]).all()                         # the deeper masked positions do not count
    assert (got[8192][:, :, :8191] == got[8193][:, :, :8191]).all()
    assert (got[8192][:, :, 8191] == got[8193][:, :, 8191:8193].sum(axis=-1)).all() and got[8192][:, :, 8191].sum() == 4
    acc_r, hist_r, _ = b.genome_coverage(bounds, genome, 2, mask_edges=MASK, hist_bins=4096)
    assert hist_r.shape == (2, 1, 16384) and hist_r.tobytes() == got[16384].tobytes() and acc_r.tobytes() == acc.tobytes()
    b.close()


# ---- c. the metagenome shape: many short scaffolds, many flushes per tile ----
@pytest.mark.parametrize("M", [1, 3])
def test_genome_hist_metagenome_shape(ctx, M):
    """300 scaffolds of 205 .. 260 positions (5 .. 60 counted each, ~17 per tile) in 40 genomes with shuffled, scattered ids: exact
    against numpy.  Renumbered so that genomes hold consecutive scaffolds, the histogram's median and n equal the sort-based
    isx_batch_summarize_genomes -- two device implementations against each other and both against numpy."""
    rng = np.random.Generator(np.random.PCG64(300 + M))
    lens = rng.integers(205, 261, 300)
    bounds = np.r_[0, np.cumsum(lens)].astype(np.int64)
    n_pos = int(bounds[-1])
    genome = rng.permutation(40)[rng.integers(0, 40, 300)].astype(np.int32)
    assert len(np.unique(genome)) > 30 and (np.diff(genome) < 0).any()
    gpos, mm, _ = _reads(rng, bounds, 3, M)
    base = rng.integers(0, 4, len(gpos)).astype(np.uint8)
    cov = _cov_levels(gpos, mm, n_pos, M)
    b = _batch(ctx, rng.integers(0, 4, n_pos).astype(np.uint8), bounds, gpos, base, mm, M)
    exp_acc, exp_hist = genome_ref.coverage_rows_flat(cov, bounds, genome, 40, mask_edges=MASK, hist_bins=64)
    acc, hist, _ = b.genome_coverage_raw(bounds, genome, 40, mask_edges=MASK, hist_bins=64)
    _assert_cov_equal(acc, hist, exp_acc, exp_hist, M)
    # consecutive genomes: 40 runs of scaffolds with random cuts
    first = np.r_[0, np.sort(rng.choice(np.arange(1, 300), 39, replace=False)), 300].astype(np.int32)
    consecutive = np.repeat(np.arange(40), np.diff(first)).astype(np.int32)
    exp_acc, exp_hist = genome_ref.coverage_rows_flat(cov, bounds, consecutive, 40, mask_edges=MASK, hist_bins=64)
    acc, hist, _ = b.genome_coverage_raw(bounds, consecutive, 40, mask_edges=MASK, hist_bins=64)
    _assert_cov_equal(acc, hist, exp_acc, exp_hist, (M, "consecutive"))
    rows, _ = b.summarize_genomes(bounds, first, mask_edges=MASK)
    b.close()
    assert (rows["n"] == acc["n"]).all() and (rows["sum_cov"] == acc["sum_cov"]).all() and (acc["n"] > 0).all()
    for g in range(40):
        for j in range(M):
            c = np.sort(cov[j, np.concatenate([np.arange(bounds[s] + MASK, bounds[s + 1] - MASK) for s in range(first[g], first[g + 1])])])
            assert _median(hist[g, j], int(acc["n"][g, j])) == int(rows["median_cov"][g, j]) == int(np.median(c)), (g, j)


# ---- d. a pipe slot gives what the batch gives ----
@pytest.mark.parametrize("M", [1, 3])
def test_slot_genome_coverage_equals_batch(ctx, M):
    """Slot.genome_coverage (what profile_bam calls) on the tile-edge layout through a read-level pipe -- dense arrays at M = 1, the
    entries layout at M = 3 -- returns the bytes of the Batch call, which equal the numpy reference"""
    bounds, genome, gpos, base, mm, pair, ref = _edge_case(M, False)
    cov = _cov_levels(gpos, mm, int(bounds[-1]), M)
    exp_acc, exp_hist = genome_ref.coverage_rows_flat(cov, bounds, genome, N_GENOMES, mask_edges=MASK, hist_bins=4096)
    b = _batch(ctx, ref, bounds, gpos, base, mm, M)
    acc, hist, _ = b.genome_coverage(bounds, genome, N_GENOMES, mask_edges=MASK)
    b.close()
    _assert_cov_equal(acc, hist, exp_acc, exp_hist, M)
    pipe, t, slot = _slot(ctx, ref, bounds, gpos, base, mm, pair, M)
    acc_s, hist_s, _ = slot.genome_coverage(bounds, genome, N_GENOMES, mask_edges=MASK)
    pipe.release(t)
    pipe.close()
    assert acc_s.tobytes() == acc.tobytes() and hist_s.tobytes() == hist.tobytes()


# ---- e. SNV level counts on synthetic rows (no batch) ----
def _snv_rows(rng, sites):
    """sites: (flat position, mm levels) in any order -> SNV_DT rows in (gpos, mm) order; allele_count over 0 .. 3 and every class"""
    gpos = np.array([p for p, lv in sorted(sites) for _ in lv], dtype=np.int64)
    rows = np.zeros(len(gpos), dtype=_lib.SNV_DT)
    rows["gpos"], rows["mm"] = gpos, [m for _, lv in sorted(sites) for m in sorted(lv)]
    rows["allele_count"], rows["cls"] = rng.integers(0, 4, len(rows)), rng.integers(0, len(util.CLASSES), len(rows))
    rows["con_base"], rows["var_base"] = rng.integers(0, 4, len(rows)), rng.integers(0, 4, len(rows))
    return rows


def _check_snv_counts(ctx, rows, bounds, n_levels):
    bounds = np.asarray(bounds, dtype=np.int64)
    got, _ = engine.snv_level_counts(ctx, rows, bounds, n_levels)
    assert got.shape == (len(bounds) - 1, n_levels)
    sc = np.searchsorted(bounds, rows["gpos"].astype(np.int64), side="right") - 1
    frame = pd.DataFrame({"position": rows["gpos"].astype(np.int64), "mm": rows["mm"].astype(np.int64),
                          "allele_count": rows["allele_count"].astype(np.int64), "class": util.CLASSES[rows["cls"]]})
    exp = np.zeros(got.shape, dtype=_lib.SNV_LEVEL_DT)
    for s in np.unique(sc):
        sdb = frame[sc == s]
        for lv in range(n_levels):
            sns, snv, div, con, pop = genome_ref.calc_snps(sdb, lv)
            exp[s, lv] = (div, sns, snv, con, pop)
    for f in exp.dtype.names:
        assert (got[f] == exp[f]).all(), (f, np.argwhere(got[f] != exp[f])[:5])
    return got


def test_snv_level_counts_block_edges_and_level_gaps(ctx):
    """255, 256 and 257 rows (one lane per row, 256 per block) with a position whose rows {0, 3, 7} lie across the block edge; levels
    with gaps under n_levels 9; rows on the first and the last position of neighbouring scaffolds, one of them a single position"""
    rng = np.random.Generator(np.random.PCG64(5))
    bounds = [0, 50, 51, 400, 1000, 5000]
    fixed = [0, 49, 50, 51, 399, 400, 999, 1000]
    free = rng.choice(np.setdiff1d(np.arange(1, 4000), fixed), 128 - len(fixed), replace=False).tolist()
    sizes = ([1, 2, 3] * 42 + [1, 1])                               # 254 rows on 128 positions, then the straddling position
    sites = [(p, sorted(rng.choice(9, k, replace=False).tolist())) for p, k in zip(sorted(fixed + free), sizes)]
    sites.append((4999, [0, 3, 7]))
    rows = _snv_rows(rng, sites)
    assert len(rows) == 257 and (rows["gpos"][254:] == 4999).all() and rows["gpos"][253] != 4999
    assert set(rows["allele_count"]) == {0, 1, 2, 3} and set(rows["cls"]) == set(range(6))
    for n in (255, 256, 257):
        got = _check_snv_counts(ctx, rows[:n], bounds, 9)
    assert (np.diff(got["divergent"].astype(np.int64), axis=1) >= 0).all() and got["divergent"][1].max() == 1 and got["divergent"][4, 8] > 0


@pytest.mark.parametrize("n_levels", [1, 40])
def test_snv_level_counts_one_and_forty_levels(ctx, n_levels):
    rng = np.random.Generator(np.random.PCG64(40 + n_levels))
    pos = np.sort(rng.choice(3000, 300, replace=False))
    sites = [(int(p), sorted(rng.choice(n_levels, int(rng.integers(1, min(n_levels, 4) + 1)), replace=False).tolist())) for p in pos]
    got = _check_snv_counts(ctx, _snv_rows(rng, sites), [0, 700, 701, 1500, 3000], n_levels)
    assert got["divergent"][:, -1].sum() == 300


def test_snv_level_counts_many_scaffolds_and_large_flat_space(ctx):
    """2 000 scaffolds, most without rows, rows on first and last positions; and a flat space of 4.2e9 positions with rows on both
    sides of 2**31 and of the scaffold bounds there (uint32 positions against int64 bounds)"""
    rng = np.random.Generator(np.random.PCG64(2000))
    bounds = np.r_[0, np.cumsum(rng.integers(1, 80, 2000))].astype(np.int64)
    used = rng.choice(2000, 60, replace=False)
    sites = {}
    for s in used:
        for p in {int(bounds[s]), int(bounds[s + 1]) - 1, int(rng.integers(bounds[s], bounds[s + 1]))}:
            sites[p] = sorted(rng.choice(4, int(rng.integers(1, 4)), replace=False).tolist())
    got = _check_snv_counts(ctx, _snv_rows(rng, list(sites.items())), bounds, 4)
    assert (got["divergent"][:, -1] > 0).sum() == 60
    big = [0, 1_000_000, 2 ** 31 + 5, 3_000_000_000, 4_200_000_000]
    at = [999_999, 1_000_000, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 4, 2 ** 31 + 5, 2_999_999_999, 3_000_000_000, 4_199_999_999]
    rows = _snv_rows(rng, [(p, sorted(rng.choice(5, int(rng.integers(1, 4)), replace=False).tolist())) for p in at])
    got = _check_snv_counts(ctx, rows, big, 5)
    assert got["divergent"][:, -1].tolist() == [1, 4, 2, 2]
    with pytest.raises(engine.IsxError) as ei:                     # the documented limit: 2**32 positions
        engine.snv_level_counts(ctx, rows, big[:-1] + [2 ** 32 + 1], 5)
    assert ei.value.code == -1


# ---- f. LD level sums on synthetic rows (no batch) ----
LD_COUNTS = [0, 1, 63, 64, 65, 129, 1000, 70, 90]                   # rows per scaffold; the last two: every r2 NaN, NaN and finite mixed


def _ld_rows(rng, counts, n_levels, starts=None):
    """LD_DT rows in (a, b, mm) order: scaffold s gets counts[s] rows; a pair's rows (1 .. 3 levels, with gaps) lie together, and in a
    scaffold of 65 rows or more one pair has its rows on lanes 62, 63 and 0 of the 64-row stride -> (rows, bounds)"""
    out, bounds = [], [0]
    for s, n in enumerate(counts):
        s0 = bounds[-1] if starts is None else starts[s]
        a, tot = s0, 0
        while tot < n:
            k = 1 if n_levels == 1 else 2 if tot < 62 else 3 if tot == 62 else int(rng.integers(1, 4))
            k = min(k, n - tot)
            a += int(rng.integers(1, 4))
            b = a + int(rng.integers(1, 60))
            for m in sorted(rng.choice(n_levels, k, replace=False).tolist()):
                out.append((a, b, m))
            tot += k
        if starts is None:
            bounds.append(a + 100)
    rows = np.zeros(len(out), dtype=_lib.LD_DT)
    rows["gpos_a"], rows["gpos_b"], rows["mm"] = [x[0] for x in out], [x[1] for x in out], [x[2] for x in out]
    rows["r2"], rows["d_prime"] = rng.random(len(rows)), rng.random(len(rows))
    rows["r2"][rng.random(len(rows)) < 0.1] = np.nan
    rows["d_prime"][rng.random(len(rows)) < 0.1] = np.nan
    return rows, np.array(bounds, dtype=np.int64)


def _check_ld_sums(ctx, rows, bounds, n_levels):
    got, _ = engine.ld_level_sums(ctx, rows, bounds, n_levels)
    again, _ = engine.ld_level_sums(ctx, rows, bounds, n_levels)
    assert got.tobytes() == again.tobytes() and got.shape == (len(bounds) - 1, n_levels)
    sc = np.searchsorted(bounds, rows["gpos_a"].astype(np.int64), side="right") - 1
    ldb = pd.DataFrame({"scaffold": sc, "position_A": rows["gpos_a"].astype(np.int64), "position_B": rows["gpos_b"].astype(np.int64),
                        "mm": rows["mm"].astype(np.int64), "r2": rows["r2"], "d_prime": rows["d_prime"]})
    exp = genome_ref.ld_rows(ldb, list(range(len(bounds) - 1)), list(range(n_levels)))
    for f in ("n", "n_r2", "n_dprime", "sum_distance"):
        assert (got[f] == exp[f]).all(), (f, np.argwhere(got[f] != exp[f])[:5])
    # float sums: n terms added in some fixed order, against math.fsum of the same terms -- (n - 1) * 2**-53 * sum |x| bounds recursive
    # summation in any order, one more ulp for fsum's own rounding
    for lv in range(n_levels):
        odb = ldb[ldb["mm"] <= lv].sort_values("mm").drop_duplicates(subset=["scaffold", "position_A", "position_B"], keep="last")
        for s, df in odb.groupby("scaffold"):
            for f, col in (("sum_r2", "r2"), ("sum_dprime", "d_prime")):
                x = df[col].to_numpy(np.float64)
                x = x[~np.isnan(x)]
                ref = math.fsum(x)
                tol = max(len(x) - 1, 0) * 2.0 ** -53 * math.fsum(np.abs(x)) + np.spacing(abs(ref))
                assert abs(float(got[f][s, lv]) - ref) <= tol, (f, s, lv, float(got[f][s, lv]), ref, tol)
    return got


@pytest.mark.parametrize("n_levels", [1, 12])
def test_ld_level_sums_lane_stride_and_nan(ctx, n_levels):
    """0, 1, 63, 64, 65, 129 and 1 000 rows per scaffold around the 64-lane stride, a pair whose rows fall on lanes 63 and 0 (the
    look-ahead to the next row crosses lanes), a scaffold whose every r2 is NaN with finite d_prime and one that mixes them"""
    rng = np.random.Generator(np.random.PCG64(64 + n_levels))
    rows, bounds = _ld_rows(rng, LD_COUNTS, n_levels)
    first = np.searchsorted(rows["gpos_a"].astype(np.int64), bounds)
    assert np.diff(first).tolist() == LD_COUNTS
    k7, k8 = slice(first[7], first[8]), slice(first[8], first[9])
    rows["r2"][k7], rows["d_prime"][k7] = np.nan, rng.random(LD_COUNTS[7])
    rows["r2"][k8][::3] = np.nan
    rows["d_prime"][k8][1::4] = np.nan
    if n_levels > 1:
        i = first[6] + 63                                           # lanes 63 and 0 of the 1 000-row scaffold: one pair
        assert rows["gpos_a"][i] == rows["gpos_a"][i + 1] and rows["gpos_b"][i] == rows["gpos_b"][i + 1] and rows["mm"][i] < rows["mm"][i + 1]
    got = _check_ld_sums(ctx, rows, bounds, n_levels)
    assert (got["n_r2"][7] == 0).all() and (got["sum_r2"][7] == 0.0).all() and (got["n_dprime"][7] == got["n"][7]).all() and got["n"][7, -1] > 0
    assert 0 < got["n_r2"][8, -1] < got["n"][8, -1] and not any(got[f][0].any() for f in got.dtype.names)
    assert got["n"][1].max() == 1 and got["n"][1, -1] == 1


def test_ld_level_sums_large_flat_space(ctx):
    """a flat space of 4.2e9 positions: a pair more than 2**31 apart (sum_distance is int64 of uint32 positions) and rows above 2**31"""
    rng = np.random.Generator(np.random.PCG64(31))
    bounds = np.array([0, 100, 4_100_000_000, 4_200_000_000], dtype=np.int64)
    rows, _ = _ld_rows(rng, [5, 70, 66], 6, starts=[0, 150, 4_100_000_000])
    far = np.flatnonzero(rows["gpos_a"].astype(np.int64) >= 150)[:3]
    rows["gpos_b"][far] = [4_000_000_000, 4_000_000_000, 4_099_999_999][:len(far)]
    o = np.lexsort((rows["mm"], rows["gpos_b"], rows["gpos_a"]))
    rows = rows[o]
    assert (rows["gpos_b"].astype(np.int64) - rows["gpos_a"].astype(np.int64)).max() > 2 ** 31 and rows["gpos_a"].max() > 2 ** 31
    got = _check_ld_sums(ctx, rows, bounds, 6)
    assert got["sum_distance"][1, -1] > 2 ** 32 and got["n"][2, -1] > 0


# ---- g. the gene pass's coverage half over many scaffolds ----
# (length, coverage): "full" = reads everywhere, "first" / "last" = eight observations on that one position, "none" = no reads
GENE_SCAFFOLDS = [(3000, "full"), (1, "full"), (30, "full"), (63, "full"), (64, "full"), (65, "full"),
                  (10, "full"), (20, "full"), (40, "full"), (50, "full"), (62, "full"),            # a run of five below the 64-position stride
                  (691, "full"),                                                                    # ends on flat 4096 (4095 / 4097 in the siblings)
                  (300, "full"), (200, "first"), (150, "full"), (200, "last"), (150, "full"),
                  (200, "none"), (130, "last"), (170, "none"), (150, "full"), (5003, "full"), (1200, "full")]


def _gene_layout(ln, kind):
    """gene (start, end) pairs of a scaffold, scaffold coordinates (inclusive ends)"""
    if ln >= 600:
        return [(0, 128), (ln - 65, ln - 1), (ln - 30, ln + 20), (ln + 5, ln + 40), (200, 200), (300, 362), (400, 463), (500, 564)]
    if kind == "first":
        return [(0, 10), (1, 20)]
    if kind == "last":
        return [(ln - 5, ln - 1), (0, ln - 2)]
    if kind == "none" and ln == 200:
        return [(0, 50), (100, 150)]
    return {1: [(0, 0)], 63: [(0, 62)], 65: [(0, 64), (10, 80)], 40: [(5, 39), (39, 39)]}.get(ln, [])


def _gene_case(M, shift):
    lens = [ln for ln, _ in GENE_SCAFFOLDS]
    lens[0] += shift
    bounds = np.r_[0, np.cumsum(lens)].astype(np.int64)
    assert bounds[12] == TILE + shift
    rng = np.random.Generator(np.random.PCG64(900 + 10 * M + shift))
    full = [i for i, (_, k) in enumerate(GENE_SCAFFOLDS) if k == "full"]
    gpos, mm, pair = _reads(rng, bounds, 8, M, read_len=20, skip=[i for i in range(len(lens)) if i not in full])
    for i, (_, k) in enumerate(GENE_SCAFFOLDS):
        if k in ("first", "last"):
            p = int(bounds[i]) if k == "first" else int(bounds[i + 1]) - 1
            gpos = np.r_[gpos, np.full(8, p)]
            mm = np.r_[mm, rng.integers(0, M, 8)]
            pair = np.r_[pair, int(pair.max()) + 1 + np.arange(8)].astype(np.uint32)
    o = np.argsort(gpos, kind="stable")
    gpos, mm, pair = gpos[o], mm[o], pair[o]
    seq = "".join(rng.choice(list("ACGT"), int(bounds[-1])))
    ref = engine.encode_seq(seq)
    base = np.where(rng.random(len(gpos)) < 0.9, ref[gpos], rng.integers(0, 4, len(gpos))).astype(np.uint8)
    names = ["sc%02d" % i for i in range(len(lens))]
    s2i, s2s = {}, {}
    for i in reversed(range(len(lens))):                            # the gene set lists the scaffolds in another order than the batch
        lay = _gene_layout(lens[i], GENE_SCAFFOLDS[i][1])
        if lay:
            g = ["%s_g%d" % (names[i], k + 1) for k in range(len(lay))]
            s2i[names[i]] = pd.DataFrame({"gene": g, "scaffold": names[i], "direction": "1", "partial": False,
                                          "start": [a for a, _ in lay], "end": [b for _, b in lay]})
            s2s[names[i]] = {n: "A" * (b - a + 1) for n, (a, b) in zip(g, lay)}
    return bounds, names, gpos, base, mm, pair, seq, ref, s2i, s2s


def _gene_expected(bounds, names, gpos, base, mm, pair, seq, s2i, M):
    """per scaffold: the oracle's entries of that scaffold's observations -> covT / clonT -> tests/gene_ref.py; and the per-position
    arrays behind the raw rows: (genes_coverage, genes_clonality, has_clon [M, n_pos], clon [M, n_pos])"""
    from oracle import oracle
    lut, fb = util.load_lut()
    n_pos = int(bounds[-1])
    has = np.zeros((M, n_pos), dtype=bool)
    clon = np.zeros((M, n_pos), dtype=np.float64)
    covs, clons = [], []
    for i, nme in enumerate(names):
        s0, s1 = int(bounds[i]), int(bounds[i + 1])
        k = (gpos >= s0) & (gpos < s1)
        e = oracle.profile_split(gpos[k] - s0, base[k], mm[k], pair[k], seq[s0:s1], 0, lut, fb)["entries"]
        covT, clonT = {}, {}
        for m in np.unique(e["mm"]):
            x = e[e["mm"] == m]
            tot = x["cnt"].sum(axis=1)
            if (tot > 0).any():
                covT[int(m)] = pd.Series(tot[tot > 0], index=x["pos"][tot > 0].astype(np.int64))
            ok = ~np.isnan(x["clon"])
            if ok.any():
                clonT[int(m)] = pd.Series(x["clon"][ok].astype(np.float32), index=x["pos"][ok].astype(np.int64))
                for j in range(int(m), M):
                    has[j, s0 + x["pos"][ok]] = True
        for m in sorted(clonT):                                     # the latest clonality of a position at every level
            for j in range(m, M):
                clon[j, s0 + clonT[m].index.to_numpy()] = clonT[m].to_numpy(np.float64)
        if nme in s2i:
            covs.append(gene_ref.gene_coverage(s2i[nme], covT))
            clons.append(gene_ref.gene_clonality(s2i[nme], clonT))
    return pd.concat([c for c in covs if len(c)]), pd.concat([c for c in clons if len(c)]), has, clon


@pytest.mark.parametrize("shift", [0, -1, 1])
@pytest.mark.parametrize("M", [1, 3])
def test_gene_coverage_half_many_scaffolds(ctx, M, shift):
    """isx_batch_profile_genes on a flat space of 23 scaffolds -- 1, 30, 63, 64, 65 positions, a run below the 64-position stride of
    k_scaffold_any, a bound on flat 4096 (4095 / 4097: shift), scaffolds covered on their first or last position only or nowhere, one of
    5 003 -- with genes at 0, at len - 1, past the end (clipped; the length in the denominators is not), beyond the end (zero rows), of
    1, 63, 64, 65 and 129 positions, overlapping, on uncovered scaffolds; the gene set lists the scaffolds in reverse.  Tables against
    tests/gene_ref.py on the oracle's per-scaffold entries, raw rows against numpy, flags per scaffold and level, two calls and (shift 0)
    a pipe slot byte for byte."""
    bounds, names, gpos, base, mm, pair, seq, ref, s2i, s2s = _gene_case(M, shift)
    n_pos = int(bounds[-1])
    exp_cov, exp_clon, has, clon = _gene_expected(bounds, names, gpos, base, mm, pair, seq, s2i, M)
    cov = _cov_levels(gpos, mm, n_pos, M)
    b = _batch(ctx, ref, bounds, gpos, base, mm, M, pair=pair)
    gs = gene_profile.GeneSet(ctx, s2i, s2s)
    gf, gl = gs.call(names, bounds)
    rows, flags, _ = b.profile_genes(gs.genes, bounds, gf, gl)
    rows2, flags2, _ = b.profile_genes(gs.genes, bounds, gf, gl)
    assert rows.tobytes() == rows2.tobytes() and flags.tobytes() == flags2.tobytes()
    # the tables
    t = gene_profile.coverage_tables(gs, names, rows, flags)
    gc, gn = t["genes_coverage"], t["genes_clonality"]
    assert list(gc["gene"]) == list(exp_cov["gene"]) and list(gc["mm"]) == list(exp_cov["mm"])
    assert np.array_equal(gc["coverage"].to_numpy(np.float64), exp_cov["coverage"].to_numpy(np.float64))
    assert np.array_equal(gc["breadth"].to_numpy(np.float64), exp_cov["breadth"].to_numpy(np.float64))
    assert list(gn["gene"]) == list(exp_clon["gene"]) and list(gn["mm"]) == list(exp_clon["mm"])
    assert np.array_equal(gn["breadth_minCov"].to_numpy(np.float64), exp_clon["breadth_minCov"].to_numpy(np.float64))
    x, y = gn["nucl_diversity"].to_numpy(np.float64), exp_clon["nucl_diversity"].to_numpy(np.float64)
    assert np.array_equal(np.isnan(x), np.isnan(y)) and np.allclose(x[~np.isnan(y)], y[~np.isnan(y)], rtol=1e-12, atol=1e-15)
    # the raw rows, in call order: the batch's scaffolds, each one's genes
    w = 0
    for i, nme in enumerate(names):
        ln = int(bounds[i + 1] - bounds[i])
        for a, e in _gene_layout(ln, GENE_SCAFFOLDS[i][1]):
            lo, hi = int(bounds[i]) + a, int(bounds[i]) + min(e, ln - 1) + 1        # empty when the gene starts beyond the scaffold
            for j in range(M):
                r = rows[w, j]
                c, h = cov[j, lo:hi] if hi > lo else cov[j, :0], has[j, lo:hi] if hi > lo else has[j, :0]
                assert (int(r["sum_cov"]), int(r["nonzero"]), int(r["counted"])) == (int(c.sum()), int((c > 0).sum()), int(h.sum())), (nme, a, e, j)
                terms = clon[j, lo:hi][h] if hi > lo else clon[j, :0]
                exact = math.fsum(terms)
                tol = max(len(terms) - 1, 0) * 2.0 ** -53 * math.fsum(np.abs(terms)) + np.spacing(abs(exact))
                assert abs(float(r["sum_clon"]) - exact) <= tol, (nme, a, e, j, float(r["sum_clon"]), exact, tol)
            w += 1
    assert w == len(rows)
    # the flags: cumulative coverage anywhere / a clonality anywhere, scaffold by scaffold
    for i in range(len(names)):
        s = slice(int(bounds[i]), int(bounds[i + 1]))
        for j in range(M):
            f = int(flags[i, j])
            assert bool(f & _lib.GENE_COV_ANY) == bool(cov[j, s].any()) and bool(f & _lib.GENE_CLON_ANY) == bool(has[j, s].any()), (i, j, f)
    assert flags[18, -1] & _lib.GENE_COV_ANY and not (flags[17] | flags[19]).any()       # covered on its last position, between uncovered ones
    assert flags[13, -1] & _lib.GENE_COV_ANY and flags[15, -1] & _lib.GENE_COV_ANY
    if shift == 0:
        pipe, tk, slot = _slot(ctx, ref, bounds, gpos, base, mm, pair, M)
        rows3, flags3, _ = slot.profile_genes(gs.genes, bounds, gf, gl)
        pipe.release(tk)
        pipe.close()
        assert rows3.tobytes() == rows.tobytes() and flags3.tobytes() == flags.tobytes()
    b.close()
    gs.close()


# ---- h. the gene pass's SNV half in a flat space beyond 2**31 ----
def test_gene_snv_half_beyond_two_to_the_31(ctx):
    """profile_snv_table on two scaffolds whose bounds lie above 2**31 (the flat space is laid out from the gene and SNV coordinates,
    nothing of its size is allocated, so the public path reaches it): for_covering's uint32 positions, int64 bounds and its backward
    loop.  A gene ends on the last position of the first scaffold, one starts on the first position of the second; the second
    scaffold's first SNV belongs to its own gene only; an intergenic SNV of the second scaffold looks back 300 positions (its longest
    gene), across the bound, and must stop there.  Expected: tests/gene_ref.py snv_tables."""
    rng = np.random.default_rng(31)
    LA = 2 ** 31 + 1000
    layout = {"big": [(10, 99, '1'), (LA - 60, LA - 1, '1'), (LA - 200, LA - 141, '-1')],
              "next": [(0, 89, '-1'), (200, 499, '1'), (450, 520, '1')]}
    s2i, s2s = {}, {}
    for sc, genes in layout.items():
        rws = []
        for i, (a, e, d) in enumerate(genes):
            name = "%s_%d" % (sc, i + 1)
            rws.append((name, sc, d, False, a, e))
            s2s.setdefault(sc, {})[name] = ''.join(rng.choice(list('ACGT'), e - a + 1))
        s2i[sc] = pd.DataFrame(rws, columns=['gene', 'scaffold', 'direction', 'partial', 'start', 'end'])
    snv = []
    for sc, ps in (("big", [5, 10, 50, 99, 100, LA - 201, LA - 200, LA - 141, LA - 140, LA - 61, LA - 60, LA - 30, LA - 1]),
                   ("next", [0, 1, 89, 90, 100, 199, 200, 449, 450, 499, 500, 520, 521, 4000])):
        for p in ps:
            lv = sorted(rng.choice(5, rng.integers(1, 4), replace=False).tolist())
            for m in lv:
                con, var = rng.choice(list('ACGT'), 2, replace=False)
                snv.append((sc, p, m, con, var, int(rng.choice([1, 2])) if m == lv[-1] else int(rng.integers(0, 4))))
    cdb = pd.DataFrame(snv, columns=['scaffold', 'position', 'mm', 'con_base', 'var_base', 'allele_count'])
    cdb['ref_base'] = 'A'
    got = gene_profile.profile_snv_table(cdb, (s2i, s2s), ctx=ctx)
    ref = gene_ref.snv_tables(cdb, s2i, s2s)
    gt, rt = keyed_types(got['SNP_mutation_types']), keyed_types(ref['SNP_mutation_types'])
    assert gt == rt and len(gt) == 27
    assert gt[("big", LA - 1)][0] in "NS" and gt[("next", 0)][0] in "NS" and gt[("next", 100)][0] == 'I'
    assert gt[("next", 450)][0] == 'M' and gt[("next", 521)][0] == 'I' and gt[("big", 5)][0] == 'I' and gt[("big", LA - 140)][0] == 'I'
    assert_counts_equal(got['genes_SNP_count'], ref['genes_SNP_count'])
    assert set(got['genes_SNP_count']['gene']) == {g for t in s2i.values() for g in t['gene']}
