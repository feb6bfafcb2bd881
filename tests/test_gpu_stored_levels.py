"""GPU: gene and genome tables from STORED profiles (isx_stored_*, k_level_sparse behind engine.StoredLevels): the gene coverage
half and the genome roll-up against the reference's goldens, the scaffold summary at the kernel's edges against tests/summary_ref.py,
profile_bam live == store_profile -> load_profile -> profile_genes_stored / genome_wide_stored end to end, and the refusals of the
device entry point."""
import os

import numpy as np
import pandas as pd
import pytest

from instrain_amd import _lib, engine
from instrain_amd.profile import gene_profile, stored
from instrain_amd.profile import genome_utilities as gu
from tests import gene_ref, genome_ref, util
from tests import summary_ref as sr

pytestmark = pytest.mark.gpu
GOLDEN = util.GOLD


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    lut, fb = util.load_lut()
    c.set_null_model(lut, fb)
    yield c
    c.close()


# ---- 1. genes against the reference ----
@pytest.mark.parametrize("case", ["synth_mm4", "synth_skipmm", "synth_offset", "c3_split"])
def test_gene_coverage_half_stored_equals_reference_golden(ctx, case):
    """covT / clonT built from the case's cov_* / clon_* arrays exactly as tests/golden/make_gene_golden.py builds them"""
    from tests.test_gpu_genes import _compare_cov, _gene_set
    gold = np.load(os.path.join(GOLDEN, "genes_cov_golden.npz"))
    g = util.load_case(case)
    seq, start = str(g["seq"]), int(g["start"])
    covT = {"s": {int(mm): pd.Series(g["cov_val"][g["cov_mm"] == mm].astype(np.int64), index=g["cov_pos"][g["cov_mm"] == mm].astype(np.int64) - start)
                  for mm in np.unique(g["cov_mm"])}}
    clonT = {"s": {int(mm): pd.Series(g["clon_val"][g["clon_mm"] == mm].astype(np.float32), index=g["clon_pos"][g["clon_mm"] == mm].astype(np.int64) - start)
                   for mm in np.unique(g["clon_mm"])}}
    pack = stored.pack_levels(["s"], [len(seq)], covT, clonT)
    assert pack["levels"].tolist() == sorted(covT["s"]) and len(pack["cov_gpos"]) == len(g["cov_pos"])
    st = engine.StoredLevels(ctx, pack)
    gs = _gene_set(ctx, [tuple(x) for x in gold[case + "__genes"]], offset=start)
    gf, gl = gs.call(["s"], pack["bounds"])
    rows, flags, ms = st.profile_genes(gs.genes, pack["bounds"], gf, gl)
    assert ms > 0 and rows.shape == (len(gold[case + "__genes"]), len(pack["levels"]))
    _compare_cov(gene_profile.coverage_tables(gs, ["s"], rows, flags, pack["levels"]), gold, case, "stored")
    rows2, flags2, _ = st.profile_genes(gs.genes, pack["bounds"], gf, gl)
    assert rows.tobytes() == rows2.tobytes() and flags.tobytes() == flags2.tobytes()        # no float atomics: identical bytes
    with pytest.raises(ValueError):
        st.profile_genes(gs.genes, [0, len(seq) - 1], gf, gl)
    st.close()
    gs.close()


# ---- 2. summaries at the edges ----
LENS = [1, 63, 64, 65, 4097]
LEVELS = [0, 1, 3]


def _edge_profile():
    """entries as (scaffold, level index, position, value) lists -> covT / clonT / clonTR dicts and the flat [M, n_pos] expectation.
    Scaffolds of 1, 63, 64, 65 and 4097 positions, adjacent; entries at position 0 and length - 1 of neighbours; s2 exists at level 3
    only; s3's key 0 has an empty series; clonalities replaced at level 3 where level 0 set them; clonTR on a handful of positions and
    one lone entry at level 1; s4 pads the coverage slices of the levels to 257, 256 and 255 entries."""
    rng = np.random.Generator(np.random.PCG64(5))
    names = ["s%d" % i for i in range(len(LENS))]
    cov = [(0, 0, 0, 7), (1, 0, 0, 3), (1, 0, 62, 9), (1, 1, 62, 2), (2, 2, 0, 4), (2, 2, 63, 5), (3, 1, 0, 6), (3, 1, 64, 1)]
    for k, extra in ((0, 254), (1, 253), (2, 253)):
        cov += [(4, k, int(p), int(v)) for p, v in zip(np.sort(rng.choice(4097, extra, replace=False)), rng.integers(1, 70000, extra))]
    clon_pos = np.sort(rng.choice(4097, 100, replace=False))
    clon = [(0, 0, 0, 0.5), (1, 0, 62, 0.75), (3, 1, 64, 1.0)] + [(4, 0, int(p), float(np.float32(1 - rng.random() * 0.9))) for p in clon_pos]
    clon += [(0, 2, 0, 0.25)] + [(4, 2, int(p), float(np.float32(1 - rng.random() * 0.9))) for p in clon_pos[::10]]      # replaced at level 3
    clon += [(2, 2, 63, 0.125)]
    clonr = [(4, 0, int(p), float(np.float32(1 - rng.random() * 0.5))) for p in (0, 1, 2048, 4095, 4096)] + [(1, 1, 0, 0.625)]
    keys = {"cov": {n: {} for n in names}, "clon": {n: {} for n in names}, "clonr": {n: {} for n in names}}
    for name, ent, dt in (("cov", cov, np.int32), ("clon", clon, np.float32), ("clonr", clonr, np.float32)):
        for s, k, p, v in ent:
            keys[name][names[s]].setdefault(LEVELS[k], ([], []))
            keys[name][names[s]][LEVELS[k]][0].append(p)
            keys[name][names[s]][LEVELS[k]][1].append(v)
        keys[name] = {n: {mm: (np.array(p, np.int64), np.array(v, dt)) for mm, (p, v) in d.items()} for n, d in keys[name].items() if d}
    keys["cov"]["s3"][0] = (np.zeros(0, np.int64), np.zeros(0, np.int32))                   # the key exists, its series is empty
    keys["clon"]["s3"][0] = (np.zeros(0, np.int64), np.zeros(0, np.float32))
    bounds = np.r_[0, np.cumsum(LENS)].astype(np.int64)
    n_pos, M = int(bounds[-1]), len(LEVELS)
    cov_l = np.zeros((M, n_pos), dtype=np.int64)
    for s, k, p, v in cov:
        cov_l[k:, bounds[s] + p] += v
    flat = lambda ent: (np.array([bounds[s] + p for s, _, p, _ in ent]), np.array([k for _, k, _, _ in ent]), np.array([v for *_, v in ent]))   # noqa: E731
    clon_l, clonr_l = sr.entry_levels(*flat(clon), n_pos, M), sr.entry_levels(*flat(clonr), n_pos, M)
    present = np.zeros((len(LENS), M), dtype=bool)
    for s, k, _, _ in cov:
        present[s, k] = True
    present[3, 0] = True
    return names, keys, bounds, cov_l, clon_l, clonr_l, present


def test_summaries_at_the_edges(ctx):
    from tests.test_gpu_summary_edges import _assert_rows, _same_but_sums
    names, keys, bounds, cov_l, clon_l, clonr_l, present = _edge_profile()
    pack = stored.pack_levels(names, LENS, keys["cov"], keys["clon"], keys["clonr"])
    assert pack["levels"].tolist() == LEVELS and np.array_equal(pack["cov_present"] != 0, present)
    assert np.diff(pack["cov_offsets"]).tolist() == [257, 256, 255] and 1 in np.diff(pack["clonr_offsets"]).tolist()
    assert pack["clon_present"][2].tolist() == [0, 0, 1] and pack["cov_present"][2].tolist() == [0, 0, 1]
    st = engine.StoredLevels(ctx, pack)
    exp = sr.scaffold_levels(cov_l, clon_l, clonr_l, present, bounds)
    rows, ms = st.summarize()
    assert ms > 0
    _assert_rows(rows, exp, "stored edges")
    again, _ = st.summarize(bounds)
    assert _same_but_sums(rows, again)
    assert rows["median_clon"][0].tolist() == [0.5, 0.5, 0.25] and rows["sum_cov"][1].tolist() == [12, 14, 14]
    assert rows["present"][3].tolist() == [1, 1, 0] and rows["nonzero"][3].tolist() == [0, 2, 2]
    with pytest.raises(ValueError):
        st.summarize(bounds[:-1])
    st.close()


# ---- 3. genome coverage against the reference ----
@pytest.fixture(scope="module")
def inp():
    d = genome_ref.load_golden_inputs()
    d["lv"], d["sv"] = genome_ref.scaffold_rows(d)
    d["ld"] = genome_ref.ld_rows(d["ldb"], d["names"], d["levels"])
    return d


def _feed_stored(ctx, gt, inp, sel):
    """tests/test_genome_info_host.py::_feed with the coverage rows from a StoredLevels object of the scaffolds `sel`"""
    names, lengths = [inp["names"][i] for i in sel], [inp["lengths"][i] for i in sel]
    pack = stored.pack_levels(names, lengths, inp["covT"], mm_values=inp["levels"])
    st = engine.StoredLevels(ctx, pack)
    ids, genomes = gt.batch_genomes(names)
    acc, hist, _ = st.genome_coverage(pack["bounds"], ids, len(genomes))
    st.close()
    e_acc, e_hist = genome_ref.coverage_rows(inp["covT"], inp["s2l"], names, ids, len(genomes), inp["levels"])
    acc, hist = acc[:len(genomes)], hist[:len(genomes)]
    for f in ("n", "sum_cov", "sumsq_cov", "max_cov"):
        assert np.array_equal(acc[f], e_acc[f]), (f, sel)
    bins = e_hist.shape[-1]
    assert np.array_equal(hist[..., :bins], e_hist) and not hist[..., bins:].any(), sel
    gt.add_batch(names, lengths, inp["lv"][sel], inp["sv"][sel], inp["ld"][sel], genomes, acc, hist, mms=inp["levels"])


def test_genome_coverage_stored_vs_reference(ctx, inp):
    assert len(inp["names"]) == 9
    one = gu.GenomeTables(inp["stb"], inp["s2l"])
    _feed_stored(ctx, one, inp, list(range(9)))
    two = gu.GenomeTables(inp["stb"], inp["s2l"])
    _feed_stored(ctx, two, inp, [0, 1, 2, 3])
    _feed_stored(ctx, two, inp, [4, 5, 6, 7, 8])               # cuts gA and gB
    for skip, name in ((False, "genome_info_golden.csv"), (True, "genome_info_golden_skipmm.csv")):
        a, b = one.genome_info(skip_mm_profiling=skip), two.genome_info(skip_mm_profiling=skip)
        genome_ref.assert_same_table(a, pd.read_csv(os.path.join(GOLDEN, name)), "stored, one object")
        pd.testing.assert_frame_equal(a, b, check_exact=True)


# ---- 4. live == stored, end to end ----
def _same_frame(got, exp, what, rtol=1e-12):
    """row and column order and every integer / object column exact; float columns within rtol (double atomics in another order)"""
    assert list(got.columns) == list(exp.columns) and len(got) == len(exp), (what, list(got.columns), list(exp.columns), len(got), len(exp))
    for c in exp.columns:
        g, e = got[c].to_numpy(), exp[c].to_numpy()
        if e.dtype.kind == "f" and len(e):
            g = g.astype(np.float64)
            assert np.array_equal(np.isnan(g), np.isnan(e)), (what, c)
            k = ~np.isnan(e)
            assert np.allclose(g[k], e[k], rtol=rtol, atol=0), (what, c, g, e)
        else:
            assert all((a == b) or (a != a and b != b) for a, b in zip(g.tolist(), e.tolist())), (what, c, g, e)


def _genes(seqs):
    layout = {"scafA": [(0, 98, '1'), (90, 200, '-1'), (2400, 2499, '1')],        # an overlap, a gene at the scaffold's end
              "scafB": [(10, 120, '1')], "scafC": [(100, 400, '-1')]}
    s2i, s2s = {}, {}
    for sc, genes in layout.items():
        rows = []
        for i, (a, b, d) in enumerate(genes):
            name = "%s_%d" % (sc, i + 1)
            s = seqs[sc][a:b + 1]
            s2s.setdefault(sc, {})[name] = gene_ref.revcomp(s) if d == '-1' else s
            rows.append((name, sc, d, False, a, b))
        s2i[sc] = pd.DataFrame(rows, columns=['gene', 'scaffold', 'direction', 'partial', 'start', 'end'])
    return s2i, s2s


@pytest.mark.parametrize("skip_mm", [False, True])
def test_live_equals_stored_end_to_end(ctx, tmp_path, skip_mm, monkeypatch):
    import instrain_amd.profile as prof
    from tests.test_gpu_genome_info import _bam
    refs, seqs, path, model = _bam(tmp_path)
    stb = {"scafA": "g1", "scafB": "g2", "scafC": "g1", "scafE": "g2", "scafF": "g1"}       # scafD: in no genome
    genes = _genes(seqs)
    live_blocks = []
    finish = engine.IRep.finish
    monkeypatch.setattr(engine.IRep, "finish", lambda self: (live_blocks.append(self.blocks()), finish(self))[1])
    st, gt, gg, rt = {}, {}, {}, {}
    splits = prof.profile_bam(path, stb=stb, genes=genes, gene_tables=gg, genome_tables=gt, scaffold_tables=st, read_tables=rt, s2s=seqs,
                              null_model=model, min_cov=5, min_freq=0.05, min_snp=10, min_read_ani=0.9, window_length=1000, ctx=ctx,
                              skip_mm_profiling=skip_mm, batch_positions=4000, strict=True)
    assert len(live_blocks) == 1 and len(gg["genes_coverage"]) > 0 and len(gg["SNP_mutation_types"]) > 0 and len(gt["genome_info"]) >= 2
    folder = str(tmp_path / "raw_data")
    stored.store_profile(folder, splits, scaffold2length=dict(refs))
    profile = stored.load_profile(folder)
    s2l = profile["scaffold2length"]
    assert list(s2l) == [n for n, _ in refs] and len(profile["raw_linkage_table"]) > 0 and len(profile["cumulative_snv_table"]) > 0
    assert len(stored.chunk_scaffolds(list(s2l), list(s2l.values()), 4000)) >= 2
    # the gene tables
    log = []
    got = gene_profile.profile_genes_stored(ctx, profile, genes, s2l, max_positions=4000, log_lines=log)
    assert sorted(got) == sorted(gene_profile.TABLE_NAMES + ["genes_table"])
    for k in gene_profile.TABLE_NAMES + ["genes_table"]:
        pd.testing.assert_frame_equal(got[k].reset_index(drop=True), gg[k].reset_index(drop=True), check_exact=True, obj=k)
    info = gene_profile.gene_info(got, got["genes_table"])
    pd.testing.assert_frame_equal(info, gene_profile.gene_info(gg, gg["genes_table"]), check_exact=True)
    # genome_info, the scaffold tables on the way, iRep's block sums
    st2, blocks = {}, []
    gw = gu.genome_wide_stored(ctx, profile, stb, s2l, fasta=seqs, mapping_info=rt["mapping_info"], skip_mm_profiling=skip_mm,
                               max_positions=4000, scaffold_tables=st2, irep_blocks=blocks)
    assert gw["scaffold2bin"] == gt["scaffold2bin"] and gw["bin2length"] == gt["bin2length"]
    assert any(c.startswith("reads_") for c in gt["genome_info"].columns) and ("mm" in gw["genome_info"].columns) == (not skip_mm)
    _same_frame(gw["genome_info"], gt["genome_info"], "genome_info")
    for c in gt["genome_info"].columns:
        if c.startswith("reads_") or c == "filtered_read_pair_count":
            assert gw["genome_info"][c].equals(gt["genome_info"][c]), c
    assert len(blocks) == 1 and all(np.array_equal(a, b) for a, b in zip(blocks[0], live_blocks[0])) and live_blocks[0][0].sum() > 0
    assert sorted(st2) == sorted(st)
    for n in st:
        _same_frame(st2[n], st[n], "scaffold table " + n)
    # ... and stored.scaffold_table on its own
    st3 = stored.scaffold_table(ctx, profile, s2l, scaffolds=list(st), max_positions=4000)
    for n in st:
        _same_frame(st3[n], st[n], "stored.scaffold_table " + n)
    # without a fasta the iRep columns are NaN and nothing else moves
    plain = gu.genome_wide_stored(ctx, profile, stb, s2l, skip_mm_profiling=skip_mm, max_positions=4000)["genome_info"]
    assert plain["iRep"].isna().all()
    keep = [c for c in plain.columns if c not in ("iRep", "iRep_GC_corrected")]
    _same_frame(plain[keep], gt["genome_info"][keep], "genome_info without a fasta")


# ---- 5. refusals on the device entry point ----
def _small_pack():
    covT = {"a": {0: (np.array([0, 5, 9]), np.array([1, 3, 2])), 2: (np.zeros(0, np.int64), np.zeros(0, np.int64))},
            "b": {5: (np.array([1, 4]), np.array([7, 8]))}}
    clonT = {"a": {0: (np.array([0, 5]), np.array([1.0, 0.5], np.float32))}, "b": {5: (np.array([4]), np.array([0.25], np.float32))}}
    return stored.pack_levels(["a", "b", "c"], [10, 6, 4], covT, clonT)


def test_refusals_leave_the_context_usable(ctx):
    good = _small_pack()

    def valid_call():
        st = engine.StoredLevels(ctx, good)
        rows, _ = st.summarize()
        st.close()
        assert rows["sum_cov"][:, -1].tolist() == [6, 15, 0] and rows["present"].tolist() == [[1, 1, 0], [0, 0, 1], [0, 0, 0]]

    def refused(code, needle, **change):
        p = dict(good)
        p.update(change)
        with pytest.raises(engine.IsxError) as e:
            engine.StoredLevels(ctx, p)
        assert e.value.code == code and needle in str(e.value), str(e.value)
        valid_call()

    valid_call()
    refused(-1, "cov_gpos", cov_gpos=np.array([5, 0, 9, 11, 14], np.uint32))                       # descending positions
    refused(-1, "cov_gpos", cov_gpos=np.array([0, 5, 9, 11, 20], np.uint32))                       # a position at bounds[n_scaffolds]
    refused(-1, "cov_present", cov_present=np.array([[1, 1, 0], [0, 0, 0], [0, 0, 0]], np.uint8))  # a series under an absent key
    refused(-1, "clon_values", clon_values=np.array([1.0, 0.0, 0.25], np.float32))
    refused(-1, "clon_values", clon_values=np.array([1.0, np.nan, 0.25], np.float32))
    refused(-1, "cov_offsets", cov_offsets=np.array([0, 3, 2, 5], np.int64))
    refused(-1, "levels", levels=np.array([0, 5, 2], np.int32))                                    # levels that do not ascend
    many = stored.pack_levels(["a"], [10], {"a": {0: (np.array([1]), np.array([1]))}}, mm_values=list(range(129)))
    with pytest.raises(engine.IsxError) as e:
        engine.StoredLevels(ctx, many)
    assert e.value.code == _lib.ERR_CAPACITY and "128" in str(e.value)
    valid_call()
    # iRep from a stored profile needs the reference codes
    irep = engine.IRep(ctx, [10, 6], [0, 0], 1, mask_edges=0)
    bare = engine.StoredLevels(ctx, good)
    with pytest.raises(engine.IsxError) as e:
        irep.add_stored(bare, [0, 1, -1], 2)
    assert e.value.code == -6 and "ref_codes" in str(e.value)
    bare.close()
    codes = np.array([0, 1, 2, 3, 4] * 4, np.uint8)
    with_ref = engine.StoredLevels(ctx, good, ref_codes=codes)
    assert irep.add_stored(with_ref, [0, 1, -1], 2) >= 0
    cov, gc, seen = irep.blocks()
    assert int(cov.sum()) == 1 + 3 + 2 + 7 + 8 and int(gc.sum()) == int(np.isin(codes[:16], (1, 3)).sum()) and seen.tolist() == [1, 1]
    with pytest.raises(engine.IsxError) as e:                                                      # a scaffold twice
        irep.add_stored(with_ref, [0, -1, -1], 2)
    assert e.value.code == -6
    with_ref.close()
    irep.close()
    valid_call()
