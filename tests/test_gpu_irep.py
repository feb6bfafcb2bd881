"""GPU: iRep on the device (isx_irep_*, engine.IRep).  Block sums exact against numpy on layouts that put scaffold interiors, block
edges, genome edges and tile edges where the kernel can go wrong; level selection and both reference layouts; additivity over batches
and ranks, byte for byte; the finishing kernels on block sums loaded directly, against the fp64 restatement (tests/irep_ref.py); the
golden genomes end to end against the reference's values (tests/golden/make_irep_golden.py); refused calls.  Expected coverage is
np.bincount of the observations."""
import numpy as np
import pytest

from instrain_amd import _lib, engine
from instrain_amd.profile import genome_utilities as gu
from tests import irep_ref, util
from tests.test_gpu_rollup_edges import _batch, _cov_levels, _reads, _slot
from tests.test_irep_host import assert_columns_equal

pytestmark = pytest.mark.gpu
INT_FIELDS = ("L", "n_windows", "n_kept", "sum_cov", "num_contigs", "flags")
FLOAT_FIELDS = ("avg_cov", "fragMbp", "kept_windows", "r2", "raw_irep", "gc_irep", "irep")


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    lut, fb = util.load_lut()
    c.set_null_model(lut, fb)
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden():
    return irep_ref.load_golden()


def expected_blocks(cov, ref, bounds, genome, n_genomes, mask=100):
    """numpy statement of the block arrays: cov / ref per flat position of a layout whose scaffolds are the set's scaffolds in order"""
    lengths = np.diff(bounds)
    gens, order, _ = irep_ref.layout(lengths, genome, n_genomes, mask)
    per_c = [cov[bounds[i]:bounds[i + 1]] for i in range(len(lengths))]
    per_g = [((ref[bounds[i]:bounds[i + 1]] == 1) | (ref[bounds[i]:bounds[i + 1]] == 3)).astype(np.int64) for i in range(len(lengths))]
    bc, bg = [], []
    for d in gens:
        mine = order[d["first_scaffold"]:d["first_scaffold"] + d["num_contigs"]]
        bc.append(irep_ref.block_sums(irep_ref.genome_array(per_c, lengths, mine, mask)))
        bg.append(irep_ref.block_sums(irep_ref.genome_array(per_g, lengths, mine, mask)))
    return np.concatenate(bc).astype(np.uint64), np.concatenate(bg).astype(np.uint32), gens


# (start, end, genome): MASK 100, 28 673 positions = seven tiles and one position
LAYOUT = [
    (0, 437, 0),                                # interior 237: starts a genome, ends in the middle of block 2
    (437, 674, 1),                              # interior 37: wholly inside one block
    (674, 873, 0), (873, 1073, 0), (1073, 1274, 0),     # 199 (dropped), 200 (nothing), 201 (one position)
    (1274, 1700, 2), (1700, 2100, 1), (2100, 2500, -1), (2500, 2950, 2), (2950, 3400, 1),       # interleaved genomes and no genome in one tile
    (3400, 3996, 0),
    (3996, 9000, 1),                            # interior begins exactly at 4096, crosses the tile edge 8192
    (9000, 12189, 2),
    (12189, 22190, 0),                          # the longest of genome 0: comes first in its array; spans three tiles
    (22190, 24576, 3),                          # ends on a tile edge; genome 3 follows genome 2 in the block array
    (24576, 28672, -1),                         # a tile of no genome
    (28672, 28673, 3),                          # the last tile holds one position
]
N_GENOMES = 5                                   # genome 4 has no scaffold


def _case(M, seed=0, non_acgt=True):
    bounds = np.array([s for s, _, _ in LAYOUT] + [LAYOUT[-1][1]], dtype=np.int64)
    genome = np.array([g for _, _, g in LAYOUT], dtype=np.int32)
    rng = np.random.Generator(np.random.PCG64(4000 + M + seed))
    gpos, mm, pair = _reads(rng, bounds, 3, M)
    base = rng.integers(0, 4, len(gpos)).astype(np.uint8)
    ref = rng.integers(0, 4, int(bounds[-1])).astype(np.uint8)
    if non_acgt:
        ref[rng.choice(len(ref), 600, replace=False)] = 4
        ref[4090:4100] = 4
    return bounds, genome, gpos, base, mm, pair, ref


def _new(ctx, bounds, genome, n_genomes=N_GENOMES):
    return engine.IRep(ctx, np.diff(bounds), genome, n_genomes)


# ---- blocks ----
@pytest.mark.parametrize("M", [1, 3])
def test_blocks_exact_at_block_genome_and_tile_edges(ctx, M):
    """every level of a batch (and level -1: G+C counts alone) against numpy, on the layout above; the seen flags; two accumulators
    give the same bytes"""
    bounds, genome, gpos, base, mm, _, ref = _case(M)
    cov = _cov_levels(gpos, mm, int(bounds[-1]), M)
    b = _batch(ctx, ref, bounds, gpos, base, mm, M)
    idx = np.arange(len(genome), dtype=np.int32)
    for level in range(-1, M):
        ir = _new(ctx, bounds, genome)
        ir.add(b, bounds, idx, level)
        bc, bg, seen = ir.blocks()
        e_c, e_g, gens = expected_blocks(cov[level] if level >= 0 else np.zeros_like(cov[0]), ref, bounds, genome, N_GENOMES)
        assert ir.n_blocks == len(e_c) == sum(d["n_blocks"] for d in gens)
        assert (bc == e_c).all(), (level, np.flatnonzero(bc != e_c)[:5])
        assert (bg == e_g).all(), (level, np.flatnonzero(bg != e_g)[:5])
        assert seen.all()
        ir2 = _new(ctx, bounds, genome)
        ir2.add(b, bounds, idx, level)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(ir2.blocks(), (bc, bg, seen)))
        ir.close()
        ir2.close()
    assert gens[0]["L"] == 237 + 0 + 1 + 396 + 9801 and gens[0]["L"] % 100 and gens[4]["L"] == 0 and e_g.sum() > 0
    b.close()


def test_blocks_on_a_slot_both_reference_layouts_and_a_deep_position(ctx):
    """a pipe slot keeps the reference as a 2-bit plane with a non-ACGT plane and, without a count table, 16-bit coverage with the exact
    values of saturated positions in a list: the same bytes as the batch (a byte per reference position, exact counts), both equal to
    numpy -- with one position 70 000 deep"""
    bounds, genome, gpos, base, mm, pair, ref = _case(1, seed=5)
    deep = 12289 + 150                          # inside the interior of the longest scaffold
    gpos = np.r_[gpos, np.full(70000, deep)]
    pair = np.r_[pair, int(pair.max()) + 1 + np.arange(70000)].astype(np.uint32)
    base = np.r_[base, np.zeros(70000, np.uint8)]
    o = np.argsort(gpos, kind="stable")
    gpos, pair, base = gpos[o], pair[o], base[o]
    mm = np.zeros(len(gpos), dtype=np.int64)
    cov = _cov_levels(gpos, mm, int(bounds[-1]), 1)
    assert cov[0, deep] > 65535
    e_c, e_g, _ = expected_blocks(cov[0], ref, bounds, genome, N_GENOMES)
    idx = np.arange(len(genome), dtype=np.int32)
    b = _batch(ctx, ref, bounds, gpos, base, mm, 1)
    ir = _new(ctx, bounds, genome)
    ir.add(b, bounds, idx, 0)
    got = ir.blocks()
    b.close()
    ir.close()
    assert (got[0] == e_c).all() and (got[1] == e_g).all()
    segs = util.reassemble_segs(gpos.astype(np.uint32), base, mm, pair)
    for want_counts in (True, False):
        pipe = engine.Pipe(ctx, max_pos=len(ref), max_obs=0, max_segs=segs.n_seg, max_splits=len(bounds), depth=1, host_threads=2,
                           n_mm_bins=1, enable_linkage=False, want_counts=want_counts)
        t = pipe.submit_reads(ref, bounds, segs)
        slot = pipe.collect(t)["slot"]
        ir = _new(ctx, bounds, genome)
        ir.add(slot, bounds, idx, 0)
        via = ir.blocks()
        pipe.release(t)
        pipe.close()
        ir.close()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(via, got)), want_counts


def test_blocks_on_a_slot_with_levels(ctx):
    bounds, genome, gpos, base, mm, pair, ref = _case(3, seed=9)
    cov = _cov_levels(gpos, mm, int(bounds[-1]), 3)
    idx = np.arange(len(genome), dtype=np.int32)
    pipe, t, slot = _slot(ctx, ref, bounds, gpos, base, mm, pair, 3)
    for level in (0, 1, 2):
        ir = _new(ctx, bounds, genome)
        ir.add(slot, bounds, idx, level)
        bc, bg, _ = ir.blocks()
        ir.close()
        e_c, e_g, _ = expected_blocks(cov[level], ref, bounds, genome, N_GENOMES)
        assert (bc == e_c).all() and (bg == e_g).all(), level
    pipe.release(t)
    pipe.close()


# ---- additivity ----
@pytest.mark.parametrize("M", [1, 3])
def test_genome_cut_over_two_batches_and_two_ranks(ctx, M):
    """the set's scaffolds split over two batches in another order than the set's, so that genome 0's and genome 1's blocks are
    shared between them (scaffolds of one genome straddle a block): either order of adding, and one rank's blocks() added into another
    rank's accumulator, give the bytes of the single batch"""
    bounds, genome, gpos, base, mm, _, ref = _case(M, seed=2)
    n_sc = len(genome)
    idx = np.arange(n_sc, dtype=np.int32)
    whole = _batch(ctx, ref, bounds, gpos, base, mm, M)
    level = M - 1
    one = _new(ctx, bounds, genome)
    one.add(whole, bounds, idx, level)
    exp = one.blocks()
    one.close()
    whole.close()
    parts = []
    for sel in ([i for i in range(n_sc) if i % 2 == 0][::-1], [i for i in range(n_sc) if i % 2 == 1]):
        lens = np.diff(bounds)[sel]
        pb = np.r_[0, np.cumsum(lens)].astype(np.int64)
        pieces = [(gpos >= bounds[i]) & (gpos < bounds[i + 1]) for i in sel]
        g = np.concatenate([gpos[k] - bounds[i] + pb[j] for j, (i, k) in enumerate(zip(sel, pieces))])
        parts.append((_batch(ctx, np.concatenate([ref[bounds[i]:bounds[i + 1]] for i in sel]), pb, g, np.concatenate([base[k] for k in pieces]),
                             np.concatenate([mm[k] for k in pieces]), M), pb, np.array(sel, dtype=np.int32)))
    for order in ((0, 1), (1, 0)):
        ir = _new(ctx, bounds, genome)
        for k in order:
            ir.add(parts[k][0], parts[k][1], parts[k][2], level)
        got = ir.blocks()
        ir.close()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, exp)), order
    ranks = []
    for k in (0, 1):
        ir = _new(ctx, bounds, genome)
        ir.add(parts[k][0], parts[k][1], parts[k][2], level)
        ranks.append(ir)
    assert not ranks[0].blocks()[2].all() and (ranks[0].blocks()[2] | ranks[1].blocks()[2]).all()
    ranks[0].add_blocks(*ranks[1].blocks())
    assert all(x.tobytes() == y.tobytes() for x, y in zip(ranks[0].blocks(), exp))
    with pytest.raises(engine.IsxError) as ei:                      # the same partial once more: its scaffolds are on both sides now
        ranks[0].add_blocks(*ranks[1].blocks())
    assert ei.value.code == -6
    for ir in ranks:
        ir.close()
    for p in parts:
        p[0].close()


# ---- finish, on blocks loaded directly ----
def _finish_case(ctx, lens_blocks, seed=1):
    """lens_blocks: [(L, num_contigs, blocks uint64)] one genome each, every genome one scaffold of L + 200 plus dropped ones; G+C
    counts are drawn here -> (device rows, restated rows)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    gcs = [rng.binomial(100, 0.35 + 0.2 * rng.random(len(b))).astype(np.uint32) for _, _, b in lens_blocks]
    lengths, genome = [], []
    for g, (L, nc, _) in enumerate(lens_blocks):
        lengths += [L + 200] + [150] * (nc - 1)
        genome += [g] * nc
    ir = engine.IRep(ctx, lengths, genome, len(lens_blocks))
    flat = np.concatenate([np.asarray(b, dtype=np.uint64) for _, _, b in lens_blocks]) if lens_blocks else np.zeros(0, np.uint64)
    assert ir.n_blocks == len(flat)
    ir.add_blocks(flat, np.concatenate(gcs) if gcs else None)
    rows, _ = ir.finish()
    again, _ = ir.finish()
    assert rows.tobytes() == again.tobytes()
    ir.close()
    return rows, [irep_ref.finish(b, L, nc, gc) for (L, nc, b), gc in zip(lens_blocks, gcs)]


def _assert_rows(rows, exp, tol):
    for g, e in enumerate(exp):
        for k in INT_FIELDS:
            assert int(rows[k][g]) == e[k], (g, k, int(rows[k][g]), e[k])
        for k in FLOAT_FIELDS:
            assert irep_ref.rel_diff(rows[k][g], e[k]) <= tol, (g, k, float(rows[k][g]), e[k])


def _gradient_blocks(rng, L, depth=12.0):
    x = np.arange(L, dtype=np.float64)
    mean = depth * 2.0 ** (-np.abs(x - L / 2) / (L / 2))
    return irep_ref.block_sums(rng.poisson(mean))


def test_finish_window_counts(ctx, golden):
    """1, 2, 7, 8, 3000 and 3001 windows (odd and even medians, more windows than one pass of 256 lanes), a genome with no windows
    between two with windows, all-zero blocks, an empty genome; integers equal, floats within ten times the recorded band of the
    restatement; two calls give identical bytes"""
    tol = 10 * golden[1]["measured_band"]
    rng = np.random.Generator(np.random.PCG64(50))
    cases = []
    for W, nc in ((1, 1), (2, 1), (7, 1), (0, 2), (8, 1), (3000, 2), (3001, 1)):
        L = 4000 if W == 0 else 5000 + 100 * (W - 1) + int(rng.integers(0, 100))
        cases.append((L, nc, _gradient_blocks(rng, L)))
    cases.append((20050, 1, np.zeros(201, dtype=np.uint64)))       # all-zero blocks
    cases.append((0, 1, np.zeros(0, dtype=np.uint64)))             # L == 0
    cases.append((30000, 3, _gradient_blocks(rng, 30000, 3.0)))    # avg_cov < 5
    rows, exp = _finish_case(ctx, cases)
    _assert_rows(rows, exp, tol)
    assert [int(x) for x in rows["n_windows"][:7]] == [1, 2, 7, 0, 8, 3000, 3001]
    assert rows["flags"][3] & _lib.IREP_FAIL_FRAG and rows["flags"][3] & _lib.IREP_NO_FIT and np.isnan(rows["irep"][3])
    assert rows["flags"][7] == (_lib.IREP_FAIL_KEPT | _lib.IREP_FAIL_COV | _lib.IREP_NO_FIT) and rows["n_kept"][7] == 0
    assert rows["flags"][8] == (_lib.IREP_EMPTY | _lib.IREP_NO_FIT) and np.isnan(rows["avg_cov"][8])
    assert rows["flags"][9] == _lib.IREP_FAIL_COV and not np.isnan(rows["raw_irep"][9]) and np.isnan(rows["irep"][9])
    assert rows["flags"][5] == 0 and rows["irep"][5] == rows["raw_irep"][5] and 1.2 < rows["irep"][5] < 3 and 1.2 < rows["gc_irep"][5] < 3
    assert np.isnan(rows["gc_irep"][[0, 3, 7, 8]]).all() and not np.isnan(rows["gc_irep"][[2, 4, 6, 9]]).any()
    assert exp[0]["flags"] & irep_ref.NO_FIT and not exp[2]["flags"] & irep_ref.NO_FIT        # one window: no line; seven: a line


def test_finish_filter_bounds_are_exact(ctx, golden):
    """windows exactly at 16 S == med2 and at 2 S == 8 med2 are kept, one unit beyond each is dropped.  Blocks b[50 k] = v_k and zeros
    elsewhere make window 50 k equal to v_k and its 49 neighbours on either side too, so the sorted sums are known: median 1600, low
    windows 200 (kept) / 199 (dropped), high ones 12800 (kept) / 12801 (dropped)"""
    tol = 10 * golden[1]["measured_band"]
    vals = [1600] * 7 + [200, 199, 12800, 12801]
    blocks = np.zeros(50 * len(vals) + 50, dtype=np.uint64)
    blocks[49::50][:len(vals)] = vals
    L = 100 * len(blocks)
    S = irep_ref.window_sums(blocks, L)
    med = float(np.median(S))
    assert med == 1600 and (S == 200).any() and (S == 199).any() and (S == 12800).any() and (S == 12801).any()
    rows, exp = _finish_case(ctx, [(L, 1, blocks)])
    _assert_rows(rows, exp, tol)
    keep = (S > 0) & (np.maximum(S, med) / np.minimum(np.maximum(S, 1), med) <= 8)      # the reference's float test: exact on these values
    assert int(rows["n_kept"][0]) == int(keep.sum()) == len(S) - (S == 199).sum() - (S == 12801).sum() - (S == 0).sum()


# ---- the golden genomes end to end ----
def _observations(cov_levels, ref):
    """[n_levels, n_pos] per-level coverage -> observations in gpos order (base = the reference's where it is a base)"""
    gs, ms = [], []
    for lv, c in enumerate(cov_levels):
        g = np.repeat(np.arange(len(c), dtype=np.int64), c)
        gs.append(g)
        ms.append(np.full(len(g), lv, dtype=np.int64))
    g, m = np.concatenate(gs), np.concatenate(ms)
    o = np.argsort(g, kind="stable")
    g, m = g[o], m[o]
    return g, np.where(ref[g] < 4, ref[g], 0).astype(np.uint8), m


@pytest.mark.parametrize("run", ["mm013", "mm02", "skip"])
def test_golden_genomes_end_to_end(ctx, golden, run):
    """the stored coverage as observations -> two batches that cut genomes -> IRep -> finish: integers and flags equal the golden's,
    floats within ten times the band recorded between the reference and the restatement; and against the restatement itself"""
    inp, gold = golden
    r = gold["runs"][run]
    tol = 10 * gold["measured_band"]
    cov, mms = irep_ref.run_levels(inp, r)
    M = len(mms)
    gt = gu.GenomeTables(inp["stb"], dict(zip(inp["names"], (int(x) for x in inp["lengths"]))))
    names, lengths, gid = gt.irep_scaffolds()
    assert names == inp["names"]
    level = gt.irep_level(mms, M, r["skip_mm_profiling"])
    ir = engine.IRep(ctx, lengths, gid, len(gt.genomes))
    n_sc = len(names)
    cut = 2                                                         # inside genome "pass"
    for lo, hi in ((cut, n_sc), (0, cut)):
        p0, p1 = int(inp["bounds"][lo]), int(inp["bounds"][hi])
        g, base, m = _observations(cov[:, p0:p1], inp["seq"][p0:p1])
        b = _batch(ctx, inp["seq"][p0:p1], inp["bounds"][lo:hi + 1] - p0, g, base, m, M)
        ir.add(b, inp["bounds"][lo:hi + 1] - p0, np.arange(lo, hi, dtype=np.int32), level)
        b.close()
    bc, bg, seen = ir.blocks()
    rows, _ = ir.finish()
    ir.close()
    assert seen.all()
    exp = irep_ref.golden_rows(inp, r)
    _assert_rows(rows, exp, tol)
    # G+C counts: the stored sequences, N counting 0
    e_gc = expected_blocks(np.zeros(len(inp["seq"]), np.int64), inp["seq"], inp["bounds"], gid, len(gt.genomes))[1]
    assert (bg == e_gc).all() and bg.sum() > 0
    for gi, gname in enumerate(inp["genomes"]):
        acc = r["accessory"].get(gname)
        if acc is None:
            continue
        for k in ("L", "num_contigs", "n_windows", "n_kept", "sum_cov", "flags"):
            assert int(rows[k][gi]) == acc[k], (gname, k)
        if "iRep" in acc:
            got = irep_ref.accessory(rows[gi])
            for k in irep_ref.GOLDEN_FLOATS + ("unfiltered_iRep",):
                assert irep_ref.rel_diff(got[k], acc[k]) <= tol, (gname, k, got[k], acc[k])
            assert (acc["iRep"] is None) == bool(np.isnan(rows["irep"][gi]))
            if acc["iRep"] is not None:
                assert irep_ref.rel_diff(rows["irep"][gi], acc["iRep"]) <= tol


def test_profile_bam_fills_the_irep_columns(ctx, tmp_path, golden):
    """profile_bam(stb=) on a small BAM over two device batches: the iRep columns of genome_info and the accessory table equal the
    restatement applied to the run's own covT (cumulated up to mm 1), NaN pattern and flags included; irep=False leaves NaN"""
    import instrain_amd.profile as prof
    from instrain_amd.profile import profile_utilities as pu
    from tests import bamwriter
    refs = [("scafA", 9000), ("scafB", 700), ("scafC", 8100), ("scafD", 1500), ("scafE", 180), ("scafG", 4000), ("scafF", 6200)]
    rng = np.random.Generator(np.random.PCG64(321))
    seqs = {n: "".join(rng.choice(list("ACGT"), ln)) for n, ln in refs}
    path = str(tmp_path / "irep.bam")
    bamwriter.write_bam(path, refs, bamwriter.random_reads(77, refs[:6], 9000))          # scafF: no reads
    lut, fb = util.load_lut()
    model = {int(i): int(v) for i, v in enumerate(lut) if v >= 0}
    model[-1] = fb
    stb = {"scafA": "g1", "scafB": "g2", "scafC": "g1", "scafE": "g2", "scafF": "g1", "scafG": "g3", "elsewhere": "g2"}     # scafD: no genome
    kw = dict(s2s=seqs, null_model=model, min_cov=5, min_freq=0.05, min_snp=10, min_read_ani=0.9, window_length=1000, ctx=ctx,
              batch_positions=10000, strict=True)
    gt = {}
    tol = 10 * golden[1]["measured_band"]
    splits = prof.profile_bam(path, stb=stb, genome_tables=gt, irep_accessory=True, **kw)
    info, acc = gt["genome_info"], gt["iRep_accessory"]
    s2l = dict(refs)
    covT = {}
    for n, _ in refs:
        parts = sorted((k for k in splits if k.rsplit(".", 1)[0] == n), key=lambda k: int(k.rsplit(".", 1)[1]))
        if parts:
            P = pu.scaffold_profile.from_splits([splits[k] for k in parts], null_model=model)
            if P.covT:
                covT[n] = P.covT
    assert 1 in set(info["mm"])
    for genome, want in (("g1", ["scafA", "scafC", "scafF"]), ("g2", ["scafB", "scafE"]), ("g3", ["scafG"])):
        per, per_gc = [], []
        for sc in want:
            per_gc.append(np.isin(list(seqs[sc]), ["G", "C"]).astype(np.int64))
            c = np.zeros(s2l[sc], dtype=np.int64)
            for m, ser in covT.get(sc, {}).items():
                if int(m) <= 1:
                    np.add.at(c, np.asarray(ser.index, dtype=np.int64), np.asarray(ser.values, dtype=np.int64))
            per.append(c)
        lens = [s2l[sc] for sc in want]
        gens, order, _ = irep_ref.layout(lens, [0] * len(want), 1)
        e = irep_ref.finish(irep_ref.block_sums(irep_ref.genome_array(per, lens, order)), gens[0]["L"], len(want),
                            irep_ref.block_sums(irep_ref.genome_array(per_gc, lens, order)))
        a = acc[acc["genome"] == genome].iloc[0]
        for k, v in irep_ref.accessory(e).items():
            assert irep_ref.rel_diff(a[k], v) <= tol, (genome, k, a[k], v)
        assert a["iRep_GC_corrected"] is True
        sub = info[info["genome"] == genome]
        assert len(sub) and (sub["iRep_GC_corrected"] == True).all()             # noqa: E712
        if np.isnan(e["irep"]):
            assert sub["iRep"].isna().all(), genome
        else:
            assert all(irep_ref.rel_diff(x, e["irep"]) <= tol for x in sub["iRep"]), genome
    assert acc[acc["genome"] == "g1"].iloc[0]["avg_cov"] > 0 and acc[acc["genome"] == "g3"].iloc[0]["fragMbp"] > 175
    gt2 = {}
    prof.profile_bam(path, stb=stb, genome_tables=gt2, irep=False, **kw)
    assert sorted(gt2) == ["bin2length", "genome_info", "scaffold2bin"]
    assert gt2["genome_info"]["iRep"].isna().all() and gt2["genome_info"]["iRep_GC_corrected"].isna().all()
    same = [c for c in info.columns if c not in ("iRep", "iRep_GC_corrected")]
    assert info[same].equals(gt2["genome_info"][same])


def test_golden_tables_through_genome_tables(ctx, golden):
    """the device's rows in GenomeTables: the reference's two columns, row for row, on the run without an mm == 1 level too"""
    from tests.test_irep_host import _tables
    inp, gold = golden
    for run in ("mm013", "mm02", "skip"):
        r = gold["runs"][run]
        exp = irep_ref.golden_rows(inp, r)
        gens, _, _ = irep_ref.layout(inp["lengths"], inp["gid"], len(inp["genomes"]))
        cov, mms = irep_ref.run_levels(inp, r)
        top = [i for i, m in enumerate(mms) if r["skip_mm_profiling"] or m <= 1]
        c = cov[top].sum(axis=0)
        ir = engine.IRep(ctx, inp["lengths"], inp["gid"], len(inp["genomes"]))
        ir.add_blocks(expected_blocks(c, inp["seq"], inp["bounds"], inp["gid"], len(inp["genomes"]))[0])
        rows, _ = ir.finish()
        ir.close()
        gt = _tables(inp, r, exp)
        gt.set_irep(rows)
        assert_columns_equal(gt.genome_info(skip_mm_profiling=r["skip_mm_profiling"]), r, 10 * gold["measured_band"], r["skip_mm_profiling"])


# ---- refused calls ----
def test_refused_calls(ctx):
    """a lean slot, a scaffold twice (in one call and over two), a set_index out of range, bounds that do not span the batch, a level
    the batch has not, a length that is not the set's: each an error code, and the block arrays stay as they were"""
    bounds, genome, gpos, base, mm, pair, ref = _case(1, seed=3, non_acgt=False)
    idx = np.arange(len(genome), dtype=np.int32)
    b = _batch(ctx, ref, bounds, gpos, base, mm, 1)
    ir = _new(ctx, bounds, genome)
    before = ir.blocks()

    def refused(code, *a):
        with pytest.raises(engine.IsxError) as ei:
            ir.add(*a)
        assert ei.value.code == code, (ei.value, a[1:])
        assert all(x.tobytes() == y.tobytes() for x, y in zip(ir.blocks(), before))

    bad = idx.copy(); bad[3] = len(genome)                                      # noqa: E702
    refused(-1, b, bounds, bad, 0)
    bad = idx.copy(); bad[3] = -2                                               # noqa: E702
    refused(-1, b, bounds, bad, 0)
    bad = idx.copy(); bad[3] = 5                                                # noqa: E702  (the length of scaffold 5 is another)
    refused(-1, b, bounds, bad, 0)
    short = bounds.copy(); short[-1] -= 1                                       # noqa: E702
    refused(-1, b, short, idx, 0)
    refused(-1, b, bounds[::-1].copy(), idx, 0)
    refused(-1, b, bounds, idx, 1)
    refused(-1, b, bounds, idx, -2)
    ir.add(b, bounds, idx, 0)
    before = ir.blocks()
    assert before[0].any()
    refused(-6, b, bounds, idx, 0)                                              # every scaffold was added before
    one = np.full(len(genome), -1, dtype=np.int32); one[0] = 0                  # noqa: E702
    refused(-6, b, bounds, one, 0)
    ir.close()
    # the same scaffold twice in one call: two batch scaffolds of one length naming one set scaffold
    b2 = np.array([0, 400, 800], dtype=np.int64)
    rng = np.random.Generator(np.random.PCG64(8))
    g2, m2, _ = _reads(rng, b2, 3, 1)
    bb = _batch(ctx, rng.integers(0, 4, 800).astype(np.uint8), b2, g2, rng.integers(0, 4, len(g2)).astype(np.uint8), m2, 1)
    ir = engine.IRep(ctx, [400, 400], [0, 0], 1)
    before = ir.blocks()
    refused(-6, bb, b2, np.array([1, 1], dtype=np.int32), 0)
    ir.add(bb, b2, np.array([1, -1], dtype=np.int32), 0)                        # -1: not one of the set's scaffolds
    assert ir.blocks()[2].tolist() == [0, 1]
    bb.close()
    ir.close()
    # a lean slot keeps no dense coverage: refused as genome_coverage is
    segs = util.reassemble_segs(gpos.astype(np.uint32), base, mm, pair)
    pipe = engine.Pipe(ctx, max_pos=len(ref), max_obs=0, max_segs=segs.n_seg, max_splits=len(bounds), depth=1, host_threads=2, pin_threads=False,
                       n_mm_bins=1, enable_linkage=True, min_snp=20, lean_output=True)
    t = pipe.submit_reads(ref, bounds, segs)
    slot = pipe.collect(t)["slot"]
    ir = _new(ctx, bounds, genome)
    before = ir.blocks()
    with pytest.raises(engine.IsxError) as e1:
        slot.genome_coverage(bounds, genome, N_GENOMES)
    refused(e1.value.code, slot, bounds, idx, 0)
    assert e1.value.code == -6
    pipe.release(t)
    pipe.close()
    ir.close()
    b.close()
