"""CPU-only: gene profiling's host side and its checker.  The test restatement of the reference's gene rules (tests/gene_ref.py)
against the stored N5 `-g` run and the reference's own coverage functions; the prodigal parser and gene_info against the stored
tables; input refusals; the new ABI structs against their ctypes mirrors."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pandas as pd
import pytest

from instrain_amd import _lib
from instrain_amd.profile import gene_profile
from tests import gene_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def n5(name):
    return pd.read_csv(os.path.join(GOLDEN, "n5_%s.csv.gz" % name), index_col=0)


def n5_genes():
    return gene_profile.parse_prodigal_genes(os.path.join(GOLDEN, "n5_genes.fna.gz"))


def keyed_types(db):
    db = db.copy()
    db['mutation'] = db['mutation'].fillna('')
    db['gene'] = db['gene'].fillna('')
    return {(s, int(p)): (t, m, g) for s, p, t, m, g in zip(db['scaffold'], db['position'], db['mutation_type'], db['mutation'], db['gene'])}


COUNT_INTS = ['gene_length', 'divergent_site_count', 'SNS_count', 'SNS_N_count', 'SNS_S_count', 'SNV_count', 'SNV_N_count', 'SNV_S_count']


def keyed_counts(db):
    return {(g, int(mm)): r for g, mm, r in zip(db['gene'], db['mm'], db[COUNT_INTS].astype(np.int64).to_numpy())}


@pytest.fixture(scope="module")
def n5_restated():
    s2i, s2s = n5_genes()
    return gene_ref.snv_tables(n5("cumulative_snv_table"), s2i, s2s)


def test_restatement_matches_the_stored_mutation_types(n5_restated):
    got, exp = keyed_types(n5_restated['SNP_mutation_types']), keyed_types(n5("SNP_mutation_types"))
    assert len(exp) == 1650
    assert {k: got[k] for k in exp} == exp
    extra = set(got) - set(exp)
    assert all(got[k][0] == 'I' for k in extra)
    from collections import Counter
    assert Counter(v[0] for v in exp.values()) == {'N': 959, 'S': 180, 'I': 444, 'M': 67}


def test_restatement_matches_the_stored_snp_counts(n5_restated):
    got, exp_db = n5_restated['genes_SNP_count'], n5("genes_SNP_count")
    exp = keyed_counts(exp_db)
    assert len(exp) == 4679
    g = keyed_counts(got)
    assert set(g) == set(exp)
    for k in exp:
        assert (g[k] == exp[k]).all(), k
    a = got.set_index(['gene', 'mm']).loc[exp_db.set_index(['gene', 'mm']).index]
    for c in ('S_sites', 'N_sites'):
        assert np.abs(a[c].to_numpy() - exp_db[c].to_numpy()).max() <= 1.2e-13


def test_parse_prodigal_genes_matches_the_stored_genes_table():
    s2i, s2s = n5_genes()
    got = gene_profile.genes_table(s2i).reset_index(drop=True)
    exp = n5("genes_table").reset_index(drop=True)
    assert len(got) == len(exp) == 810
    assert list(got['gene']) == list(exp['gene'])
    assert list(got['scaffold']) == list(exp['scaffold'])
    assert (got['start'].to_numpy() == exp['start'].to_numpy()).all() and (got['end'].to_numpy() == exp['end'].to_numpy()).all()
    assert [str(x) for x in got['direction']] == [str(x) for x in exp['direction']]
    assert (got['partial'].to_numpy() == exp['partial'].to_numpy()).all()
    assert sum(len(v) for v in s2s.values()) == 810 and (got['direction'].astype(str) == '-1').sum() == 432


def test_gene_info_from_the_stored_tables_matches_the_tsv():
    tables = {k: n5(k) for k in ('genes_coverage', 'genes_clonality', 'genes_SNP_count')}
    got = gene_profile.gene_info(tables, n5("genes_table")).reset_index(drop=True)
    with gzip.open(os.path.join(GOLDEN, "n5_gene_info.tsv.gz"), "rt") as f:
        exp = pd.read_csv(f, sep='\t')
    assert len(got) == len(exp) == 801
    assert list(got.columns) == list(exp.columns)
    got, exp = got.set_index('gene'), exp.set_index('gene').loc[got['gene']]
    for c in exp.columns:
        if c in ('scaffold', 'direction', 'partial'):
            assert (got[c].astype(str) == exp[c].astype(str)).all(), c
        else:
            a, b = got[c].to_numpy(np.float64), exp[c].to_numpy(np.float64)
            assert (np.isnan(a) == np.isnan(b)).all(), c
            ok = ~np.isnan(a)
            assert np.allclose(a[ok], b[ok], rtol=1e-12, atol=0), c


def test_restatement_equals_reference_coverage_golden():
    gold = np.load(os.path.join(GOLDEN, "genes_cov_golden.npz"))
    for case in ("synth_mm4", "synth_skipmm", "synth_offset", "c3_split"):
        g = np.load(os.path.join(GOLDEN, case + ".npz"), allow_pickle=True)
        layout = gold[case + "__genes"]
        gdb = pd.DataFrame({"gene": np.arange(len(layout)), "start": layout[:, 0], "end": layout[:, 1]})
        covT = {int(m): pd.Series(g["cov_val"][g["cov_mm"] == m], index=g["cov_pos"][g["cov_mm"] == m]) for m in np.unique(g["cov_mm"])}
        clonT = {int(m): pd.Series(g["clon_val"][g["clon_mm"] == m].astype(np.float32), index=g["clon_pos"][g["clon_mm"] == m])
                 for m in np.unique(g["clon_mm"])}
        cov, clon = gene_ref.gene_coverage(gdb, covT), gene_ref.gene_clonality(gdb, clonT)
        a = np.stack([cov['gene'], cov['mm'], cov['coverage'], cov['breadth']], axis=1).astype(np.float64)
        assert np.array_equal(a, gold[case + "__cov"]), case
        b = np.stack([clon['gene'], clon['mm'], clon['nucl_diversity'], clon['breadth_minCov']], axis=1).astype(np.float64)
        e = gold[case + "__clon"]
        assert np.array_equal(np.isnan(b), np.isnan(e)) and np.allclose(b[~np.isnan(b)], e[~np.isnan(e)], rtol=1e-12, atol=0), case


def test_biopython_ambiguity_rule_of_the_restatement():
    assert gene_ref.translate_codon('GCN') == 'A' and gene_ref.translate_codon('NNN') == 'X'
    assert gene_ref.translate_codon('TAN') == 'X' and gene_ref.translate_codon('TAA') == '*' and gene_ref.translate_codon('CTN') == 'L'


def test_input_refusals(tmp_path):
    with pytest.raises(NotImplementedError):
        gene_profile.parse_genes(str(tmp_path / "genes.gbk"))
    with pytest.raises(NotImplementedError):
        gene_profile.parse_genes(str(tmp_path / "genes.gb"))
    with pytest.raises(ValueError):
        gene_profile.parse_genes(str(tmp_path / "genes.txt"))
    bad = tmp_path / "bad.fna"
    bad.write_text(">sc_1_1 # 1 # 6 # 1 # ID=1_1;partial=00\nATGaaa\n")
    with pytest.raises(ValueError, match="sc_1_1"):
        gene_profile.parse_genes(str(bad))
    short = tmp_path / "short.fna"
    short.write_text(">sc_1_1 # 1 # 9 # -1 # ID=1_1;partial=00\nATGAAA\n")
    with pytest.raises(ValueError, match="sc_1_1"):
        gene_profile.parse_genes(str(short))
    ok = tmp_path / "ok.fa"
    ok.write_text(">sc_1_1 # 1 # 6 # -1 # ID=1_1;partial=01\nATG\nNAA\n>sc_1_2 # 10 # 12 # 1 # x\nTAA\n")
    s2i, s2s = gene_profile.parse_genes(str(ok))
    assert list(s2i) == ['sc_1'] and s2s['sc_1']['sc_1_1'] == 'ATGNAA'
    t = s2i['sc_1']
    assert list(t['start']) == [0, 9] and list(t['end']) == [5, 11] and list(t['direction']) == ['-1', '1'] and list(t['partial']) == [True, False]


def test_gene_struct_sizes_match_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "instrain_amd.h"\nint main(void){printf("%zu %zu %zu %zu\\n",'
                   'sizeof(isx_gene),sizeof(isx_gene_cov),sizeof(isx_gene_snv_count),sizeof(isx_gene_mutation));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [_lib.GENE_DT.itemsize, _lib.GENE_COV_DT.itemsize, _lib.GENE_SNV_COUNT_DT.itemsize, _lib.GENE_MUTATION_DT.itemsize]
    assert C.sizeof(C.c_double) == 8
