#!/usr/bin/env python3
"""
tests/golden/make_gene_golden.py -- the gene-profiling fixtures (`inStrain profile -g`).

Runs ONLY where the reference is (like make_golden.py, whose stub importer it uses).  It
  1. copies the stored tables of the reference's own `-g` run (test_data/N5_271_010G1_scaffold_min1000.fa-vs-N5_271_010G1.forRC.IS:
     cumulative_snv_table, genes_table, genes_coverage, genes_clonality, genes_SNP_count, SNP_mutation_types, gene_info.tsv) and
     the gene file next to it (gzipped) into tests/golden/n5_*;
  2. writes genes_cov_golden.npz: the reference's own calc_gene_coverage / calc_gene_clonality (GeneProfile.py:352-422) applied to
     the covT / clonT stored in synth_*.npz / c3_split.npz, with hand-made gene layouts (overlaps, genes at both scaffold ends, a
     gene without coverage, a gene past the scaffold end; mm > 0 and skip-mm cases).
Nothing of the reference's source text is stored -- only data.

usage: python tests/golden/make_gene_golden.py
"""
import gzip
import os
import shutil
import sys

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402

REF = make_golden.REF
N5 = os.path.join(REF, "test", "test_data", "N5_271_010G1_scaffold_min1000.fa-vs-N5_271_010G1.forRC.IS")
N5_FNA = os.path.join(REF, "test", "test_data", "N5_271_010G1_scaffold_min1000.fa.genes.fna")
N5_TABLES = ["cumulative_snv_table", "genes_table", "genes_coverage", "genes_clonality", "genes_SNP_count", "SNP_mutation_types"]

# (fixture, gene layouts as (start, end) in scaffold coordinates, inclusive)
COV_CASES = {
    "synth_mm4": [(0, 98), (50, 250), (240, 240), (300, 399), (350, 460), (120, 131)],
    "synth_skipmm": [(0, 98), (50, 250), (300, 399), (350, 460), (399, 399)],
    "synth_offset": [(20000, 20098), (20050, 20250), (20300, 20399), (20350, 20460)],
    "c3_split": [(0, 1199), (1100, 2300), (5000, 5002), (9900, 9998), (9960, 9998), (9990, 10500)],
}


def copy_n5():
    for name in N5_TABLES:
        shutil.copyfile(os.path.join(N5, "raw_data", name + ".csv.gz"), os.path.join(HERE, "n5_%s.csv.gz" % name))
    src = os.path.join(N5, "output", os.path.basename(N5) + "_gene_info.tsv")
    for a, b in ((src, "n5_gene_info.tsv.gz"), (N5_FNA, "n5_genes.fna.gz")):
        with open(a, "rb") as f, open(os.path.join(HERE, b), "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0) as g:
            g.write(f.read())


def cov_golden():
    make_golden.import_reference()
    import inStrain.GeneProfile as gp
    out = {}
    for case, layout in COV_CASES.items():
        g = np.load(os.path.join(HERE, case + ".npz"), allow_pickle=True)
        covT = {int(mm): pd.Series(g["cov_val"][g["cov_mm"] == mm].astype(np.int64), index=g["cov_pos"][g["cov_mm"] == mm].astype(np.int64))
                for mm in np.unique(g["cov_mm"])}
        clonT = {int(mm): pd.Series(g["clon_val"][g["clon_mm"] == mm].astype(np.float32), index=g["clon_pos"][g["clon_mm"] == mm].astype(np.int64))
                 for mm in np.unique(g["clon_mm"])}
        gdb = pd.DataFrame({"gene": ["%s_%d" % (case, i + 1) for i in range(len(layout))],
                            "start": [a for a, _ in layout], "end": [b for _, b in layout]})
        cdb = gp.calc_gene_coverage(gdb, covT)
        ldb = gp.calc_gene_clonality(gdb, clonT)
        gi = {n: i for i, n in enumerate(gdb["gene"])}
        out[case + "__genes"] = np.array(layout, dtype=np.int64)
        out[case + "__cov"] = np.stack([cdb["gene"].map(gi).to_numpy(np.float64), cdb["mm"].to_numpy(np.float64),
                                        cdb["coverage"].to_numpy(np.float64), cdb["breadth"].to_numpy(np.float64)], axis=1)
        out[case + "__clon"] = np.stack([ldb["gene"].map(gi).to_numpy(np.float64), ldb["mm"].to_numpy(np.float64),
                                         ldb["nucl_diversity"].to_numpy(np.float64), ldb["breadth_minCov"].to_numpy(np.float64)], axis=1)
    np.savez_compressed(os.path.join(HERE, "genes_cov_golden.npz"), **out)


if __name__ == "__main__":
    copy_n5()
    cov_golden()
    print("gene fixtures written to", HERE)
