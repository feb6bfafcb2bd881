"""GPU: the device passes behind genome_info (isx_batch_genome_coverage, isx_snv_level_counts, isx_ld_level_sums) against the
oracle's / pandas restatements of the reference's rules, and profile_bam(stb=...) end to end against tests/genome_ref.py."""
import os

import numpy as np
import pandas as pd
import pytest

from instrain_amd import _lib, engine
from instrain_amd.profile import genome_utilities as gu
from instrain_amd.profile import profile_utilities as pu
from tests import genome_ref, util

pytestmark = pytest.mark.gpu
GOLDEN = util.GOLD
LENS = [5200, 150, 199, 201, 2600, 900, 1301, 7001]
SCAFFOLD_GENOME = [0, 1, 0, -1, 2, 1, 0, 2]


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    lut, fb = util.load_lut()
    c.set_null_model(lut, fb)
    yield c
    c.close()


def _close(x, e):
    return (np.isnan(x) and np.isnan(e)) or abs(x - e) <= 1e-9 * max(1.0, abs(e))


def _observations(mm_levels):
    """coverage ~ 12 on every scaffold but the 900 one (no reads); mm levels random"""
    sb = np.r_[0, np.cumsum(LENS)].astype(np.int64)
    rng = np.random.Generator(np.random.PCG64(11 + mm_levels))
    pos = np.sort(np.concatenate([sb[i] + rng.integers(0, ln, size=12 * ln) for i, ln in enumerate(LENS) if ln != 900])).astype(np.int64)
    return sb, pos, rng.integers(0, 4, len(pos)).astype(np.uint8), rng.integers(0, mm_levels, len(pos)), rng.integers(0, 4, int(sb[-1])).astype(np.uint8)


def _batch(ctx, sel, sb, pos, base, mm, ref, mm_levels):
    """the scaffolds `sel` (consecutive) as a batch of their own -> (Batch, its scaffold bounds)"""
    lo, hi = int(sb[sel[0]]), int(sb[sel[-1] + 1])
    k = (pos >= lo) & (pos < hi)
    bounds = (sb[sel[0]:sel[-1] + 2] - lo).astype(np.int64)
    b = engine.Batch(ctx, ref[lo:hi], bounds, engine.pack_obs((pos[k] - lo).astype(np.uint32), base[k], mm[k]), None, n_mm_bins=mm_levels,
                     enable_linkage=False)
    b.run()
    return b, bounds


def _median(hist_row, n):
    cum = np.cumsum(hist_row.astype(np.int64))
    lo, hi = int((cum > (n - 1) // 2).argmax()), int((cum > n // 2).argmax())
    return int((lo + hi) / 2.0)


@pytest.mark.parametrize("mm_levels", [1, 4])
def test_genome_coverage_vs_oracle(ctx, mm_levels):
    """scattered genomes (interleaved scaffolds, one scaffold in no genome, 150 / 199 / 201 positions around the 2 x 100 masked ones, one
    without reads): counts, sums and the histogram's median exact, std / SEM within the summation-order bound; a short histogram's
    catch-all bin and the exact repeat; two batches cutting genome 0 add up to the one-batch result element for element"""
    from oracle import summary
    sb, pos, base, mm, ref = _observations(mm_levels)
    names = ["s%d" % i for i in range(len(LENS))]
    b, bounds = _batch(ctx, list(range(len(LENS))), sb, pos, base, mm, ref, mm_levels)
    acc, hist, ms = b.genome_coverage(bounds, SCAFFOLD_GENOME, 3, mask_edges=100)
    assert hist.shape == (3, mm_levels, 4096) and ms > 0
    covT = {}
    for i, nme in enumerate(names):
        k = (pos >= sb[i]) & (pos < sb[i + 1])
        covT[nme] = {m: np.unique(pos[k & (mm == m)] - sb[i], return_counts=True) for m in range(mm_levels)}
    g2s = {"g%d" % g: [n for n, x in zip(names, SCAFFOLD_GENOME) if x == g] for g in range(3)}
    exp = summary.genome_coverage_rows(covT, dict(zip(names, LENS)), g2s, list(range(mm_levels)), mask_edges=100)
    covs = {}
    for g in range(3):
        for m in range(mm_levels):
            series = {n: {l: pd.Series(v, index=p) for l, (p, v) in c.items()} for n, c in covT.items()}
            covs[g, m] = genome_ref.masked_coverage(series, dict(zip(names, LENS)), g2s["g%d" % g], m).astype(np.int64)
            c, a, e = covs[g, m], acc[g, m], exp[g * mm_levels + m]
            assert e["genome"] == "g%d" % g and e["mm"] == m
            assert (int(a["n"]), int(a["sum_cov"]), int(a["sumsq_cov"]), int(a["max_cov"])) == (len(c), int(c.sum()), int((c * c).sum()), int(c.max()))
            assert (hist[g, m] == np.bincount(c, minlength=4096)).all()
            n, s, q = int(a["n"]), int(a["sum_cov"]), int(a["sumsq_cov"])
            ss = (n * q - s * s) / n
            assert _median(hist[g, m], n) == e["coverage_median"]
            assert _close(float(np.sqrt(ss / n)), e["coverage_std"]) and _close(float(np.sqrt(ss / (n - 1)) / np.sqrt(n)), e["coverage_SEM"])
    assert acc["n"][0, 0] == 5000 + 0 + 1101 and acc["n"][1, 0] == 0 + 700 and acc["n"][2, 0] == 2400 + 6801
    # 8 bins: the raw call says so (max_cov) and keeps a catch-all last bin; the method comes back exact
    acc8, hist8, _ = b.genome_coverage_raw(bounds, SCAFFOLD_GENOME, 3, mask_edges=100, hist_bins=8)
    assert (acc8["max_cov"] >= 8).any() and (acc8 == acc).all()
    for g in range(3):
        for m in range(mm_levels):
            assert hist8[g, m, 7] == int((covs[g, m] >= 7).sum()) and (hist8[g, m, :7] == hist[g, m, :7]).all()
    acc_r, hist_r, _ = b.genome_coverage(bounds, SCAFFOLD_GENOME, 3, mask_edges=100, hist_bins=8)
    top = int(acc["max_cov"].max())
    assert hist_r.shape[-1] == 1 << top.bit_length() and (acc_r == acc).all()
    assert (hist_r == hist[:, :, :hist_r.shape[-1]]).all() and not hist[:, :, hist_r.shape[-1]:].any()
    # bad arguments are refused before anything is touched
    for bad in (dict(scaffold_genome=[0, 1, 0, -1, 2, 1, 0, 3]), dict(scaffold_genome=[0, 1, 0, -2, 2, 1, 0, 2]), dict(hist_bins=1),
                dict(bounds=np.r_[bounds[:-1], bounds[-1] - 1]), dict(bounds=np.r_[bounds[:3], bounds[2], bounds[4:]])):
        with pytest.raises(engine.IsxError) as ei:
            b.genome_coverage_raw(bad.get("bounds", bounds), bad.get("scaffold_genome", SCAFFOLD_GENOME), 3, hist_bins=bad.get("hist_bins", 64))
        assert ei.value.code == -1
    b.close()
    # two batches, genome 0 cut between them (s0..s2 | s3..s7): sums and padded histograms add up
    tot_acc, tot_hist = np.zeros_like(acc), np.zeros(hist.shape, dtype=np.int64)
    for sel in ([0, 1, 2], [3, 4, 5, 6, 7]):
        bb, bnd = _batch(ctx, sel, sb, pos, base, mm, ref, mm_levels)
        a, h, _ = bb.genome_coverage(bnd, [SCAFFOLD_GENOME[i] for i in sel], 3, mask_edges=100, hist_bins=32 if sel[0] == 0 else 64)
        bb.close()
        for f in ("n", "sum_cov", "sumsq_cov"):
            tot_acc[f] += a[f]
        tot_acc["max_cov"] = np.maximum(tot_acc["max_cov"], a["max_cov"])
        tot_hist[:, :, :h.shape[-1]] += h
    assert (tot_acc == acc).all() and (tot_hist == hist).all()


def _fetch_case(ctx, name, linkage=True):
    g = util.load_case(name)
    start, seq = int(g["start"]), str(g["seq"])
    p = np.asarray(g["pos"], dtype=np.int64)
    sel = (p >= start) & (p < start + len(seq))
    mm = np.asarray(g["mm"])[sel]
    n_levels = int(mm.max()) + 1
    b = engine.Batch(ctx, engine.encode_seq(seq), [0, len(seq)], engine.pack_obs((p[sel] - start).astype(np.uint32), np.asarray(g["base"])[sel], mm),
                     np.asarray(g["pair"])[sel].astype(np.uint32), n_mm_bins=n_levels, enable_linkage=linkage, min_cov=int(g["p_min_cov"]),
                     min_freq=float(g["p_min_freq"]), min_snp=int(g["p_min_snp"]))
    b.run()
    res = b.fetch()
    b.close()
    return res, len(seq), n_levels


def _snp_frame(rows):
    return pd.DataFrame({"position": rows["gpos"].astype(np.int64), "mm": rows["mm"].astype(np.int64),
                         "allele_count": rows["allele_count"].astype(np.int64), "class": np.array(pu.CLASSES)[rows["cls"]]})


def _check_snv_levels(got, rows, bounds, n_levels):
    for s in range(len(bounds) - 1):
        sdb = _snp_frame(rows[(rows["gpos"] >= bounds[s]) & (rows["gpos"] < bounds[s + 1])])
        for lv in range(n_levels):
            sns, snv, div, con, pop = genome_ref.calc_snps(sdb, lv)            # the test-owned restatement, not product code
            assert tuple(int(got[s, lv][f]) for f in ("sns", "snv", "divergent", "con", "pop")) == (sns, snv, div, con, pop), (s, lv)


@pytest.mark.parametrize("name", ["synth_mm4", "synth_dense", "synth_ambig"])
def test_snv_level_counts_vs_calc_snps(ctx, name):
    res, n_pos, n_levels = _fetch_case(ctx, name, linkage=False)
    rows = res["snv"]
    assert len(rows) > 20
    bounds = np.array([0, n_pos // 3 + 1, (2 * n_pos) // 3 - 1, n_pos], dtype=np.int64)
    got, ms = engine.snv_level_counts(ctx, rows, bounds, n_levels + 1)        # one level more than any row has: it repeats the last
    assert got.shape == (3, n_levels + 1) and ms >= 0
    _check_snv_levels(got, rows, bounds, n_levels + 1)
    assert got["divergent"].sum() > 0


def test_snv_level_counts_edges_and_coverage_table(ctx):
    res, n_pos, n_levels = _fetch_case(ctx, "synth_mm4", linkage=False)
    rows = res["snv"]
    # zero rows
    got, _ = engine.snv_level_counts(ctx, rows[:0], [0, 10, n_pos], 3)
    assert got.shape == (2, 3) and not any(got[f].any() for f in got.dtype.names)
    # a row at the last level; a scaffold (the middle one) without rows
    few = np.zeros(3, dtype=_lib.SNV_DT)
    few["gpos"], few["mm"], few["allele_count"], few["cls"] = [5, 5, n_pos - 1], [0, n_levels - 1, n_levels - 1], [2, 1, 2], [5, 2, 3]
    got, _ = engine.snv_level_counts(ctx, few, [0, 100, n_pos - 100, n_pos], n_levels)
    _check_snv_levels(got, few, [0, 100, n_pos - 100, n_pos], n_levels)
    assert not any(got[1][f].any() for f in got.dtype.names) and got[2, n_levels - 1]["snv"] == 1 and got[2, 0]["divergent"] == 0
    assert got[0, n_levels - 1]["sns"] == 1 and got[0, 0]["snv"] == 1
    # refused: a level out of range, rows out of order, bounds that do not start at 0
    bad = few.copy()
    bad["mm"][2] = n_levels
    for r, bnd in ((bad, [0, n_pos]), (few[::-1], [0, n_pos]), (few, [1, n_pos]), (few, [0, 50, 50, n_pos]), (few, [0, n_pos - 1])):
        with pytest.raises(engine.IsxError) as ei:
            engine.snv_level_counts(ctx, r, bnd, n_levels)
        assert ei.value.code == -1
    # make_coverage_table takes the device's counts instead of calc_snps: the same frame
    b_levels = np.zeros(n_levels, dtype=_lib.SCAFFOLD_LEVEL_DT)
    b_levels["mm"], b_levels["present"] = np.arange(n_levels), 1
    b_levels["nonzero"], b_levels["sum_cov"], b_levels["sumsq_cov"], b_levels["counted"], b_levels["sum_clon"] = 900, 9000, 99000, 800, 790.5
    got, _ = engine.snv_level_counts(ctx, rows, [0, n_pos], n_levels)
    sdb = _snp_frame(rows)
    pd.testing.assert_frame_equal(pu.make_coverage_table(b_levels, n_pos, "s", sdb, snv_counts=got[0]), pu.make_coverage_table(b_levels, n_pos, "s", sdb),
                                  check_exact=True)


def _ld_frame(rows, bounds):
    sc = np.searchsorted(np.asarray(bounds), rows["gpos_a"].astype(np.int64), side="right") - 1
    return pd.DataFrame({"scaffold": sc, "position_A": rows["gpos_a"].astype(np.int64), "position_B": rows["gpos_b"].astype(np.int64),
                         "distance": rows["gpos_b"].astype(np.int64) - rows["gpos_a"].astype(np.int64), "mm": rows["mm"].astype(np.int64),
                         "r2": rows["r2"], "d_prime": rows["d_prime"]})


def _check_ld_levels(ctx, rows, bounds, n_levels):
    got, ms = engine.ld_level_sums(ctx, rows, bounds, n_levels)
    again, _ = engine.ld_level_sums(ctx, rows, bounds, n_levels)
    assert got.tobytes() == again.tobytes()                                    # fixed summation order
    ldb = _ld_frame(rows, bounds)
    for lv in range(n_levels):                                                 # _genome_wide_linkage, a scaffold as a genome
        odb = ldb[ldb["mm"] <= lv].sort_values("mm").drop_duplicates(subset=["scaffold", "position_A", "position_B"], keep="last")
        groups = dict(list(odb.groupby("scaffold")))
        for s in range(len(bounds) - 1):
            r, df = got[s, lv], groups.get(s)
            if df is None:
                assert r["n"] == 0 and r["n_r2"] == 0 and r["n_dprime"] == 0 and r["sum_distance"] == 0
                continue
            assert (int(r["n"]), int(r["n_r2"]), int(r["n_dprime"]), int(r["sum_distance"])) == \
                (len(df), int(df["r2"].notna().sum()), int(df["d_prime"].notna().sum()), int(df["distance"].sum())), (s, lv)
            for n, tot, col in ((r["n_r2"], r["sum_r2"], "r2"), (r["n_dprime"], r["sum_dprime"], "d_prime")):
                assert _close(tot / n if n else np.nan, df[col].mean()), (s, lv, col)
    return got


def test_ld_level_sums_fetched_rows(ctx):
    res, n_pos, n_levels = _fetch_case(ctx, "synth_m1_ld")
    rows = res["ld"]
    assert len(rows) > 100
    got = _check_ld_levels(ctx, rows, [0, n_pos // 3, n_pos // 2, n_pos], n_levels + 1)
    assert got["n"][:, -1].sum() == len(np.unique(np.stack([rows["gpos_a"], rows["gpos_b"]]), axis=1).T)
    zero, _ = engine.ld_level_sums(ctx, rows[:0], [0, n_pos], 2)
    assert zero.tobytes() == np.zeros((1, 2), dtype=_lib.LD_LEVEL_DT).tobytes()
    bad = rows[:4].copy()
    bad["mm"][3] = n_levels
    for r, n in ((bad, n_levels), (rows[:4][::-1], n_levels)):
        with pytest.raises(engine.IsxError) as ei:
            engine.ld_level_sums(ctx, r, [0, n_pos], n)
        assert ei.value.code == -1


def test_ld_level_sums_stored_sars_table(ctx):
    """the reference's own raw_linkage_table of the sars run laid out as isx_ld rows: 26 levels, 886 rows with NaN r2"""
    db = pd.read_csv(os.path.join(GOLDEN, "sars_cov_2_raw_linkage_table.csv.gz")).sort_values(["position_A", "position_B", "mm"])
    rows = np.zeros(len(db), dtype=_lib.LD_DT)
    rows["gpos_a"], rows["gpos_b"], rows["mm"] = db["position_A"].values, db["position_B"].values, db["mm"].values
    rows["r2"], rows["d_prime"] = db["r2"].values, db["d_prime"].values
    assert int(db["mm"].max()) == 25 and int(np.isnan(rows["r2"]).sum()) == 886
    got = _check_ld_levels(ctx, rows, [0, 9000, 20000, 29903], 26)
    assert got["n"].sum() > 0 and (got["n_r2"] < got["n"]).any()


def _bam(tmp_path):
    from tests import bamwriter
    refs = [("scafA", 2500), ("scafB", 700), ("scafC", 3100), ("scafD", 1500), ("scafE", 180), ("scafF", 2200)]
    rng = np.random.Generator(np.random.PCG64(123))
    seqs = {n: "".join(rng.choice(list("ACGT"), ln)) for n, ln in refs}
    path = str(tmp_path / "genomes.bam")
    bamwriter.write_bam(path, refs, bamwriter.random_reads(31, refs[:5], 5000))           # scafF: no reads
    lut, fb = util.load_lut()
    model = {int(i): int(v) for i, v in enumerate(lut) if v >= 0}
    model[-1] = fb
    return refs, seqs, path, model


@pytest.mark.parametrize("skip_mm", [False, True])
def test_profile_bam_genome_info_end_to_end(ctx, tmp_path, skip_mm, monkeypatch):
    """two interleaved genomes over two device batches (genome g1 is cut by the batch boundary), a scaffold the stb does not name, one
    no read reaches and one the run does not hold: genome_info == the restatement applied to the run's own scaffold tables, raw
    linkage tables and covT; without stb nothing is made and the splits are the same"""
    import instrain_amd.profile as prof
    refs, seqs, path, model = _bam(tmp_path)
    stb = {"scafA": "g1", "scafB": "g2", "scafC": "g1", "scafE": "g2", "scafF": "g1", "elsewhere": "g2"}      # scafD: in no genome
    kw = dict(s2s=seqs, null_model=model, min_cov=5, min_freq=0.05, min_snp=10, min_read_ani=0.9, window_length=1000, ctx=ctx,
              skip_mm_profiling=skip_mm, batch_positions=4000, strict=True)
    st, gt, batches = {}, {}, []
    add_batch = gu.GenomeTables.add_batch
    monkeypatch.setattr(gu.GenomeTables, "add_batch", lambda self, names, *a, **k: (batches.append(list(names)), add_batch(self, names, *a, **k))[1])
    splits = prof.profile_bam(path, stb=stb, scaffold_tables=st, genome_tables=gt, **kw)
    assert len(batches) >= 2 and sum("scafA" in b or "scafC" in b or "scafF" in b for b in batches) >= 2      # g1 spans batches
    assert sorted(gt) == ["bin2length", "genome_info", "scaffold2bin"] and gt["scaffold2bin"] == stb
    assert gt["bin2length"] == {"g1": 2500 + 3100 + 2200, "g2": 700 + 180}
    names = [n for n, _ in refs]
    by_scaffold = {n: sorted((k for k in splits if k.rsplit(".", 1)[0] == n), key=lambda k: int(k.rsplit(".", 1)[1])) for n in names}
    covT, ldbs = {}, []
    for n in names:
        parts = [splits[k] for k in by_scaffold[n]]
        if not parts:
            continue
        P = pu.scaffold_profile.from_splits(parts, null_model=model)
        if P.covT:
            covT[n] = P.covT
        if len(P.raw_linkage_table):
            ldbs.append(P.raw_linkage_table)
    sdb = pd.concat([st[n] for n in names if n in st and len(st[n])]).reset_index(drop=True)
    ldb = pd.concat(ldbs).reset_index(drop=True) if ldbs else pd.DataFrame()
    assert len(ldb) > 0 and sdb["scaffold"].nunique() >= 4
    exp = genome_ref.genome_info(sdb, ldb, covT, stb, {n: ln for n, ln in refs}, skip_mm_profiling=skip_mm)
    got = gt["genome_info"]
    assert set(got["genome"]) == {"g1", "g2"} and ("mm" in got.columns) == (not skip_mm)
    genome_ref.assert_same_table(got, exp, "end to end")
    # the scaffold tables made from the device's SNV counts == the ones made by calc_snps on the host
    st2, gt2 = {}, {}
    plain = prof.profile_bam(path, scaffold_tables=st2, genome_tables=gt2, **kw)
    assert gt2 == {} and sorted(plain) == sorted(splits)
    for n in st2:
        pd.testing.assert_frame_equal(st[n], st2[n], check_exact=True)
    for k in plain:
        pd.testing.assert_frame_equal(plain[k].raw_snp_table, splits[k].raw_snp_table)
        pd.testing.assert_frame_equal(plain[k].raw_linkage_table, splits[k].raw_linkage_table)
