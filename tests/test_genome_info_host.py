"""genome_info on the host (no GPU): profile/genome_utilities.py GenomeTables against the reference's own genomeLevel_from_IS
(tests/golden/make_genome_info_golden.py), fed with per-scaffold rows derived in numpy from the golden's inputs
(tests/genome_ref.py) -- the rows the device passes deliver on a GPU."""
import ctypes as C  # noqa: F401
import os
import subprocess

import numpy as np
import pandas as pd
import pytest

from instrain_amd import _lib
from instrain_amd.profile import genome_utilities as gu
from tests import genome_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = genome_ref.GOLDEN


@pytest.fixture(scope="module")
def inp():
    d = genome_ref.load_golden_inputs()
    d["lv"], d["sv"] = genome_ref.scaffold_rows(d)
    d["ld"] = genome_ref.ld_rows(d["ldb"], d["names"], d["levels"])
    return d


def _feed(gt, inp, sel):
    """one add_batch with the scaffolds `sel` (indices in scaffold order)"""
    names = [inp["names"][i] for i in sel]
    ids, genomes = gt.batch_genomes(names)
    acc, hist = genome_ref.coverage_rows(inp["covT"], inp["s2l"], names, ids, len(genomes), inp["levels"])
    gt.add_batch(names, [inp["lengths"][i] for i in sel], inp["lv"][sel], inp["sv"][sel], inp["ld"][sel], genomes, acc, hist, mms=inp["levels"])


def _golden(skip):
    return pd.read_csv(os.path.join(GOLDEN, "genome_info_golden_skipmm.csv" if skip else "genome_info_golden.csv"))


@pytest.mark.parametrize("skip", [False, True])
def test_genome_tables_vs_reference(inp, skip):
    gt = gu.GenomeTables(inp["stb"], inp["s2l"])
    _feed(gt, inp, list(range(len(inp["names"]))))
    assert gt.bin2length == genome_ref.bin2length(inp["stb"], inp["s2l"])
    genome_ref.assert_same_table(gt.genome_info(skip_mm_profiling=skip), _golden(skip), "one batch")


@pytest.mark.parametrize("skip", [False, True])
def test_genome_spanning_two_batches(inp, skip):
    """genomes gA and gB are cut by the batch boundary; the histograms of the two batches have different lengths"""
    one = gu.GenomeTables(inp["stb"], inp["s2l"])
    _feed(one, inp, list(range(len(inp["names"]))))
    two = gu.GenomeTables(inp["stb"], inp["s2l"])
    _feed(two, inp, [0, 1, 2, 3])
    _feed(two, inp, [4, 5, 6, 7, 8])
    a, b = one.genome_info(skip_mm_profiling=skip), two.genome_info(skip_mm_profiling=skip)
    pd.testing.assert_frame_equal(a, b, check_exact=True)
    genome_ref.assert_same_table(b, _golden(skip), "two batches")


@pytest.mark.parametrize("skip", [False, True])
def test_restatement_vs_reference(inp, skip):
    """tests/genome_ref.py genome_info (what the end-to-end GPU test compares with) reproduces the golden too"""
    sdb = pd.read_csv(os.path.join(GOLDEN, "genome_info_scaffold_table.csv"))
    got = genome_ref.genome_info(sdb, inp["ldb"], inp["covT"], inp["stb"], inp["s2l"], skip_mm_profiling=skip)
    genome_ref.assert_same_table(got, _golden(skip), "restatement")


def test_no_linkage_rows_gives_nan_columns(inp):
    gt = gu.GenomeTables(inp["stb"], inp["s2l"])
    sel = list(range(len(inp["names"])))
    names = [inp["names"][i] for i in sel]
    ids, genomes = gt.batch_genomes(names)
    acc, hist = genome_ref.coverage_rows(inp["covT"], inp["s2l"], names, ids, len(genomes), inp["levels"])
    gt.add_batch(names, inp["lengths"], inp["lv"], inp["sv"], np.zeros_like(inp["ld"]), genomes, acc, hist, mms=inp["levels"])
    db = gt.genome_info()
    assert list(db.columns[-4:]) == ["SNV_distance_mean", "d_prime_mean", "linked_SNV_count", "r2_mean"]
    assert db[db.columns[-4:]].isna().all().all() and all(db[c].dtype == np.float64 for c in db.columns[-4:])


def test_inexact_histogram_is_refused(inp):
    gt = gu.GenomeTables(inp["stb"], inp["s2l"])
    names = inp["names"][:1]
    ids, genomes = gt.batch_genomes(names)
    acc, hist = genome_ref.coverage_rows(inp["covT"], inp["s2l"], names, ids, 1, inp["levels"], hist_bins=4)
    with pytest.raises(ValueError, match="not exact"):
        gt.add_batch(names, inp["lengths"][:1], inp["lv"][:1], inp["sv"][:1], inp["ld"][:1], genomes, acc, hist, mms=inp["levels"])


def test_parse_stb(tmp_path, inp):
    p = tmp_path / "x.stb"
    p.write_text("".join("%s\t%s\n" % kv for kv in inp["stb"].items()))
    assert gu.parse_stb(str(p)) == inp["stb"]
    assert gu.parse_stb(inp["stb"]) is inp["stb"]


def test_genome_struct_sizes_match_header(tmp_path):
    """sizeof() of the three roll-up structs as the C compiler sees the header == their numpy dtypes"""
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "instrain_amd.h"\nint main(void){printf("%zu %zu %zu\\n",'
                   'sizeof(isx_genome_cov),sizeof(isx_snv_level),sizeof(isx_ld_level));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    c_sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert c_sizes == [_lib.GENOME_COV_DT.itemsize, _lib.SNV_LEVEL_DT.itemsize, _lib.LD_LEVEL_DT.itemsize], c_sizes
    assert all(s in _lib.SYMBOLS for s in ("isx_batch_genome_coverage", "isx_snv_level_counts", "isx_ld_level_sums"))


@pytest.mark.parametrize("name", ["single", "double", "triple"])
def test_calc_snps_restatement_vs_reference_tables(name):
    """tests/genome_ref.py calc_snps (what the GPU tests compare isx_snv_level_counts with) against the five counts the reference's own
    make_coverage_table -> calc_snps wrote into the stored cumulative scaffold tables of the merge goldens, from the stored SNV tables
    they were made of (tests/golden/make_merge_golden.py): every level, the gap between levels 2 and 7 included.  (The divergent /
    sns / snv / con / pop integers of genome_info_inputs.npz are random draws of make_genome_info_golden.py, not counts of any SNV
    table -- on gA_1 `divergent` falls from 6 to 2 between levels 0 and 1, which no table gives -- so they cannot pin this rule.)"""
    snv = pd.read_csv(os.path.join(GOLDEN, "merge_%s_cumulative_snv_table.csv" % name))
    sdb = pd.read_csv(os.path.join(GOLDEN, "merge_%s_cumulative_scaffold_table.csv" % name))
    assert len(sdb) >= 3 and snv.duplicated("position").any()                  # positions with rows at several levels
    for _, r in sdb.iterrows():
        exp = tuple(int(r[c]) for c in ("SNS_count", "SNV_count", "divergent_site_count", "consensus_divergent_sites", "population_divergent_sites"))
        assert genome_ref.calc_snps(snv, int(r["mm"])) == exp, (name, int(r["mm"]))
    assert genome_ref.calc_snps(snv[:0], 3) == (0, 0, 0, 0, 0)


def test_coverage_rows_flat_equals_coverage_rows(inp):
    """the array form of the coverage reference == the covT form on the golden's inputs (mask 100 and 0, a short catch-all histogram)"""
    names, levels = inp["names"], inp["levels"]
    ids, genomes = gu.GenomeTables(inp["stb"], inp["s2l"]).batch_genomes(names)
    bounds = np.r_[0, np.cumsum(inp["lengths"])]
    cov = np.zeros((len(levels), int(bounds[-1])), dtype=np.int64)
    for i, n in enumerate(names):
        for m, ser in inp["covT"][n].items():
            for j, lv in enumerate(levels):
                if m <= lv:
                    np.add.at(cov[j], bounds[i] + np.asarray(ser.index), np.asarray(ser.values))
    for mask, bins in ((100, None), (0, None), (100, 8)):
        a, h = genome_ref.coverage_rows(inp["covT"], inp["s2l"], names, ids, len(genomes), levels, mask_edges=mask, hist_bins=bins)
        a2, h2 = genome_ref.coverage_rows_flat(cov, bounds, ids, len(genomes), mask_edges=mask, hist_bins=bins)
        assert a.tobytes() == a2.tobytes() and h.shape == h2.shape and (h == h2).all(), (mask, bins)
