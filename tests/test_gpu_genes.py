"""GPU: gene profiling (`inStrain profile -g`) on the device -- the SNV half against the stored N5 run and the test restatement
(tests/gene_ref.py) on synthetic traps, the coverage half through a Batch and a read-level pipe slot against the reference's own
calc_gene_coverage / calc_gene_clonality (genes_cov_golden.npz), and run-to-run byte identity."""
import os

import numpy as np
import pandas as pd
import pytest

from instrain_amd import _lib, engine
from instrain_amd.profile import gene_profile
from tests import gene_ref, util
from tests.test_genes_host import COUNT_INTS, keyed_counts, keyed_types, n5, n5_genes

pytestmark = pytest.mark.gpu
GOLDEN = util.GOLD


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    lut, fb = util.load_lut()
    c.set_null_model(lut, fb)
    yield c
    c.close()


def assert_counts_equal(got, exp):
    g, e = keyed_counts(got), keyed_counts(exp)
    assert set(g) == set(e)
    for k in e:
        assert (g[k] == e[k]).all(), (k, g[k], e[k])
    a = got.set_index(['gene', 'mm']).loc[exp.set_index(['gene', 'mm']).index]
    for c in ('S_sites', 'N_sites', 'dNdS_substitutions', 'pNpS_variants'):
        x, y = a[c].to_numpy(np.float64), exp[c].to_numpy(np.float64)
        assert (np.isnan(x) == np.isnan(y)).all(), c
        ok = ~np.isnan(x)
        assert np.allclose(x[ok], y[ok], rtol=1e-12, atol=0), c


def test_profile_snv_table_matches_the_stored_n5(ctx):
    s2i, s2s = n5_genes()
    got = gene_profile.profile_snv_table(n5("cumulative_snv_table"), (s2i, s2s), ctx=ctx)
    exp_t = keyed_types(n5("SNP_mutation_types"))
    got_t = keyed_types(got['SNP_mutation_types'])
    assert len(exp_t) == 1650 and {k: got_t[k] for k in exp_t} == exp_t
    assert all(got_t[k][0] == 'I' for k in set(got_t) - set(exp_t))
    assert_counts_equal(got['genes_SNP_count'], n5("genes_SNP_count"))
    assert len(got['genes_SNP_count']) == 4679
    assert list(got['genes_SNP_count'].columns) == gene_profile.SNP_COUNT_COLUMNS
    # and against the restatement: every row, the extra intergenic ones included
    ref = gene_ref.snv_tables(n5("cumulative_snv_table"), s2i, s2s)
    assert keyed_types(ref['SNP_mutation_types']) == got_t
    assert set(got['SNP_mutation_types'].columns) == set(ref['SNP_mutation_types'].columns)
    # two runs: identical bytes
    again = gene_profile.profile_snv_table(n5("cumulative_snv_table"), (s2i, s2s), ctx=ctx)
    for k in ('genes_SNP_count', 'SNP_mutation_types'):
        pd.testing.assert_frame_equal(got[k], again[k], check_exact=True)


def _gene_set(ctx, layout, offset=0):
    names = ["g%d" % (i + 1) for i in range(len(layout))]
    gdb = pd.DataFrame({"gene": names, "scaffold": "s", "direction": "1", "partial": False,
                        "start": [a - offset for a, _ in layout], "end": [b - offset for _, b in layout]})
    return gene_profile.GeneSet(ctx, {"s": gdb}, {"s": {n: "A" * (b - a + 1) for n, (a, b) in zip(names, layout)}})


def _compare_cov(tables, gold, case, what):
    cov, clon = tables['genes_coverage'], tables['genes_clonality']
    gi = lambda s: s.str[1:].astype(int) - 1          # noqa: E731
    a = np.stack([gi(cov['gene']), cov['mm'], cov['coverage'], cov['breadth']], axis=1).astype(np.float64)
    assert np.array_equal(a, gold[case + "__cov"]), (case, what)
    b = np.stack([gi(clon['gene']), clon['mm'], clon['nucl_diversity'], clon['breadth_minCov']], axis=1).astype(np.float64)
    e = gold[case + "__clon"]
    assert b.shape == e.shape and np.array_equal(b[:, :2], e[:, :2]) and np.array_equal(b[:, 3], e[:, 3]), (case, what)
    assert np.array_equal(np.isnan(b[:, 2]), np.isnan(e[:, 2])), (case, what)
    ok = ~np.isnan(e[:, 2])
    assert np.allclose(b[ok, 2], e[ok, 2], rtol=1e-12, atol=1e-15), (case, what)


@pytest.mark.parametrize("case", ["synth_mm4", "synth_skipmm", "synth_offset", "c3_split"])
def test_coverage_half_batch_equals_reference_golden(ctx, case):
    gold = np.load(os.path.join(GOLDEN, "genes_cov_golden.npz"))
    g = util.load_case(case)
    seq, start = str(g["seq"]), int(g["start"])
    pos = np.asarray(g["pos"], np.int64)
    sel = (pos >= start) & (pos < start + len(seq))
    M = int(np.asarray(g["mm"]).max()) + 1
    obs = engine.pack_obs((pos[sel] - start).astype(np.uint32), np.asarray(g["base"])[sel], np.asarray(g["mm"])[sel])
    kw = dict(min_cov=int(g["p_min_cov"]), min_freq=float(g["p_min_freq"]), min_snp=int(g["p_min_snp"]))
    b = engine.Batch(ctx, engine.encode_seq(seq), [0, len(seq)], obs, np.asarray(g["pair"])[sel].astype(np.uint32), n_mm_bins=M,
                     enable_linkage=False, **kw)
    b.run()
    gs = _gene_set(ctx, [tuple(x) for x in gold[case + "__genes"]], offset=start)
    bounds = np.array([0, len(seq)], np.int64)
    gf, gl = gs.call(["s"], bounds)
    rows, flags, _ = b.profile_genes(gs.genes, bounds, gf, gl)
    _compare_cov(gene_profile.coverage_tables(gs, ["s"], rows, flags), gold, case, "batch")
    rows2, flags2, _ = b.profile_genes(gs.genes, bounds, gf, gl)
    assert rows.tobytes() == rows2.tobytes() and flags.tobytes() == flags2.tobytes()        # no float atomics: identical bytes
    # a read-level pipe slot (skip-mm: dense arrays; mm on: the entries layout) gives the same rows
    if case in ("synth_skipmm", "synth_mm4"):
        segs = util.reassemble_segs(obs["gpos"], obs["base"], obs["mm"], np.asarray(g["pair"])[sel].astype(np.uint32))
        pipe = engine.Pipe(ctx, max_pos=len(seq), max_obs=0, max_segs=segs.n_seg, max_splits=2, depth=1, host_threads=2, n_mm_bins=M,
                           enable_linkage=False, want_counts=M == 1, layout=_lib.LAYOUT_MM_ENTRIES if M > 1 else 0, **kw)
        t = pipe.submit_reads(engine.encode_seq(seq), [0, len(seq)], segs)
        r = pipe.collect(t)
        rows3, flags3, _ = r["slot"].profile_genes(gs.genes, bounds, gf, gl)
        pipe.release(t)
        pipe.close()
        assert rows3.tobytes() == rows.tobytes() and flags3.tobytes() == flags.tobytes(), case
    b.close()
    gs.close()


def _rand_seq(rng, n):
    return ''.join(rng.choice(list('ACGT'), n))


def _trap_inputs():
    """four scaffolds: every trap of the SNV half.  A: + / - genes, an overlap (M), a - gene of length 101 (trailing partial codon),
    a gene with N letters (GCN / NNN codons), SNVs in first / last codons and between genes, several levels per position;
    B: genes, SNV rows whose highest-mm rows all have allele_count 0 or 3 (GeneException); C: genes, no SNV rows; D: no genes"""
    rng = np.random.default_rng(7)
    layout = {"scA": [(0, 98, '1'), (90, 200, '-1'), (300, 400, '-1'), (500, 610, '1'), (650, 652, '1')],
              "scB": [(10, 120, '1')], "scC": [(0, 59, '-1')]}
    s2i, s2s = {}, {}
    for sc, genes in layout.items():
        rows = []
        for i, (a, b, d) in enumerate(genes):
            name = "%s_%d" % (sc, i + 1)
            seq = _rand_seq(rng, b - a + 1)
            if (sc, i) == ("scA", 3):
                seq = seq[:30] + "GCN" + seq[33:60] + "NNN" + seq[63:90] + "N" + seq[91:]
            rows.append((name, sc, d, False, a, b))
            s2s.setdefault(sc, {})[name] = seq
        s2i[sc] = pd.DataFrame(rows, columns=['gene', 'scaffold', 'direction', 'partial', 'start', 'end'])
    snv = []

    def add(sc, p, levels):
        for mm, ac in levels:
            con, var = rng.choice(list('ACGT'), 2, replace=False)
            snv.append((sc, p, mm, con, var, ac))
    for p in (0, 1, 2, 3, 50, 95, 98, 99, 150, 198, 199, 200, 250, 300, 301, 302, 350, 398, 399, 400, 530, 531, 532, 561, 590, 651, 700):
        lv = sorted(rng.choice(6, rng.integers(1, 4), replace=False).tolist())
        add("scA", p, [(mm, int(rng.choice([0, 1, 1, 2, 2, 3]))) for mm in lv[:-1]] + [(lv[-1], int(rng.choice([1, 2])))])
    add("scA", 560, [(0, 2), (3, 3)])                      # highest row with allele_count 3: no type, still counted
    add("scB", 20, [(0, 1), (2, 0)])
    add("scB", 21, [(1, 3)])
    add("scD", 5, [(0, 1)])
    cdb = pd.DataFrame(snv, columns=['scaffold', 'position', 'mm', 'con_base', 'var_base', 'allele_count'])
    cdb['ref_base'] = 'A'
    return cdb, s2i, s2s


def test_snv_half_traps_equal_restatement(ctx):
    cdb, s2i, s2s = _trap_inputs()
    log_lines, ref_log = [], []
    got = gene_profile.profile_snv_table(cdb, (s2i, s2s), ctx=ctx, log_lines=log_lines)
    ref = gene_ref.snv_tables(cdb, s2i, s2s, log_lines=ref_log)
    assert log_lines == ref_log == ["DEBUG FAILURE GeneException scB"]
    gt, rt = keyed_types(got['SNP_mutation_types']), keyed_types(ref['SNP_mutation_types'])
    assert gt == rt
    kinds = {v[0] for v in gt.values()}
    assert kinds == {'I', 'M', 'N', 'S'}
    assert {k[0] for k in gt} == {"scA"}                  # B: GeneException, C: no SNV rows, D: no genes
    assert_counts_equal(got['genes_SNP_count'], ref['genes_SNP_count'])
    assert set(got['genes_SNP_count']['gene']) == set(s2i['scA']['gene'])
    # the partial codon of the length-101 minus gene and the ambiguous codons take the reference's path
    assert gt[("scA", 300)][0] == 'S'


def test_sites_equal_restatement(ctx):
    _, s2i, s2s = _trap_inputs()
    gs = gene_profile.GeneSet(ctx, s2i, s2s)
    got = gs.sites()
    exp = np.array([gene_ref.count_sites(s2s[sc][g]) for sc in s2i for g in s2i[sc]['gene']])
    assert np.array_equal(got, exp)                       # same codon order, same fp64 sums
    gs.close()


def test_profile_bam_gene_tables_equal_restatement(ctx, tmp_path):
    """profile_bam(gene_file=...) on the sars run (26 mm levels, three splits): the gene tables equal the restatement applied to the
    merged SplitObjects; a gene crosses the split bound at 10 000; without gene arguments the split objects are the same"""
    import instrain_amd.profile as prof
    from instrain_amd.profile.profile_utilities import scaffold_profile
    from tests.test_oracle_golden import read_fasta
    lut, fb = util.load_lut()
    model = {int(i): int(v) for i, v in enumerate(lut) if v >= 0}
    model[-1] = fb
    seq = read_fasta(os.path.join(GOLDEN, "sars_cov_2_MT039887.1.fasta")).upper()
    genes = [(265, 13467, '1'), (21562, 25383, '1'), (25392, 26219, '-1'), (26244, 26471, '1'), (26522, 27190, '-1'),
             (27201, 27386, '1'), (27393, 27758, '1'), (27755, 27886, '-1'), (28273, 29532, '1'), (29557, 29673, '1')]
    fna = tmp_path / "sars_genes.fna"
    with open(fna, "w") as f:
        for i, (a, b, d) in enumerate(genes):
            s = ''.join(c if c in 'ACGTN' else 'N' for c in seq[a:b + 1])
            if d == '-1':
                s = gene_ref.revcomp(s)
            f.write(">MT039887.1_%d # %d # %d # %s # ID=1_%d;partial=00\n%s\n" % (i + 1, a + 1, b + 1, d, i + 1, s))
    kw = dict(s2s={"MT039887.1": seq}, null_model=model, min_cov=5, min_freq=0.05, min_snp=20, min_read_ani=0.95, ctx=ctx)
    bam = os.path.join(GOLDEN, "sars_cov_2.sorted.bam")
    gt = {}
    splits = prof.profile_bam(bam, gene_file=str(fna), gene_tables=gt, strict=True, **kw)
    plain = prof.profile_bam(bam, **kw)
    assert sorted(splits) == sorted(plain) == ["MT039887.1.0", "MT039887.1.1", "MT039887.1.2"]
    for k in splits:
        pd.testing.assert_frame_equal(splits[k].raw_snp_table, plain[k].raw_snp_table)
    P = scaffold_profile.from_splits([splits["MT039887.1.%d" % i] for i in range(3)], null_model=model)
    s2i, s2s = gene_profile.parse_genes(str(fna))
    gdb = s2i["MT039887.1"]
    exp_cov, exp_clon = gene_ref.gene_coverage(gdb, P.covT), gene_ref.gene_clonality(gdb, P.clonT)
    assert len(np.unique(exp_cov['mm'])) == 26
    for got, exp, cols in ((gt['genes_coverage'], exp_cov, ['coverage', 'breadth']), (gt['genes_clonality'], exp_clon, ['nucl_diversity', 'breadth_minCov'])):
        assert list(got['gene']) == list(exp['gene']) and list(got['mm']) == list(exp['mm'])
        for c in cols:
            x, y = got[c].to_numpy(np.float64), exp[c].to_numpy(np.float64)
            assert (np.isnan(x) == np.isnan(y)).all(), c
            assert np.allclose(x[~np.isnan(x)], y[~np.isnan(y)], rtol=1e-12, atol=1e-15), c
    ref = gene_ref.snv_tables(P.cumulative_snv_table, s2i, s2s)
    assert keyed_types(gt['SNP_mutation_types']) == keyed_types(ref['SNP_mutation_types'])
    assert_counts_equal(gt['genes_SNP_count'], ref['genes_SNP_count'])
    assert len(gt['genes_table']) == len(genes)
    info = gene_profile.gene_info(gt, gt['genes_table'])
    assert len(info) > 0 and list(info.columns) == gene_profile.GENE_INFO_COLUMNS
    # genes only on a scaffold the BAM does not hold: the same split objects, empty gene tables, no failure line
    logs, gt2 = [], {}
    elsewhere = ({"elsewhere": gdb.assign(scaffold="elsewhere")}, {"elsewhere": s2s["MT039887.1"]})
    again = prof.profile_bam(bam, genes=elsewhere, gene_tables=gt2, logs=logs, **kw)
    assert sorted(again) == sorted(plain) and not logs
    assert len(gt2['genes_table']) == len(genes) and all(len(gt2[k]) == 0 for k in gene_profile.TABLE_NAMES)
