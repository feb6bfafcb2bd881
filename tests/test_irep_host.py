"""iRep on the host (no GPU): the layout function against a Python statement of it, the fp64 restatement (tests/irep_ref.py) against the
reference's values (tests/golden/make_irep_golden.py), and GenomeTables' two iRep columns against the reference's, row for row."""
import os
import subprocess

import numpy as np
import pytest

from instrain_amd import _lib, engine
from instrain_amd.profile import genome_utilities as gu
from tests import genome_ref, irep_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def data():
    return irep_ref.load_golden()


def _check_layout(lengths, genome, n_genomes, mask):
    gen, order, off = engine.irep_layout(lengths, genome, n_genomes, mask)
    e_gen, e_order, e_off = irep_ref.layout(lengths, genome, n_genomes, mask)
    assert order.tolist() == e_order and off.tolist() == e_off
    for g, d in enumerate(e_gen):
        for k, v in d.items():
            assert int(gen[k][g]) == v, (g, k, int(gen[k][g]), v)
    # no block belongs to two genomes
    ends = gen["first_block"] + gen["n_blocks"]
    assert (gen["first_block"][1:] == ends[:-1]).all() and gen["first_block"][0] == 0
    return gen, order, off


def test_layout_against_python_statement():
    rng = np.random.Generator(np.random.PCG64(7))
    # mask edges: 199 / 200 / 201, a genome of dropped scaffolds only, a genome without scaffolds, ties in caller order, no genome
    lengths = [5300, 199, 200, 201, 150, 180, 5300, 5199, 5200, 5201, 900, 40000, 5300]
    genome = [0, 0, 0, 0, 1, 1, 0, 3, 4, 5, -1, 5, 0]
    gen, order, off = _check_layout(lengths, genome, 7, 100)
    assert order[:3].tolist() == [0, 6, 12]                                # equal lengths: the caller's order
    assert gen["L"].tolist() == [3 * 5100 + 0 + 1, 0, 0, 4999, 5000, 5001 + 39800, 0]
    assert gen["n_windows"].tolist() == [(15301 - 5000) // 100 + 1, 0, 0, 0, 1, (44801 - 5000) // 100 + 1, 0]
    assert gen["n_blocks"][3] == 50 and gen["n_blocks"][4] == 50 and gen["num_contigs"].tolist() == [6, 2, 0, 1, 1, 2, 0]
    assert off[1] == -1 and off[3] == 3 * 5100 and off[2] == 3 * 5100 + 1 and off[10] == -1 and off[4] == -1
    for mask in (0, 1, 100, 2600):
        n = int(rng.integers(1, 60))
        _check_layout(rng.integers(1, 6000, n), rng.integers(-1, 5, n), 5, mask)


def test_layout_refuses_bad_arguments():
    for lengths, genome, n in (([10, 0], [0, 0], 1), ([10], [1], 1), ([10], [-2], 1), ([10], [0], 0)):
        with pytest.raises(engine.IsxError) as ei:
            engine.irep_layout(lengths, genome, n)
        assert ei.value.code == -1


def test_struct_sizes_match_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "instrain_amd.h"\nint main(void){printf("%zu %zu %d %d\\n",'
                   'sizeof(isx_irep_genome),sizeof(isx_irep_row),ISX_IREP_WINDOW,ISX_IREP_SLIDE);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [_lib.IREP_GENOME_DT.itemsize, _lib.IREP_ROW_DT.itemsize, _lib.IREP_WINDOW, _lib.IREP_SLIDE] == [48, 96, 5000, 100]
    assert irep_ref.WINDOW == 5000 and irep_ref.SLIDE == 100


@pytest.mark.parametrize("run", ["mm013", "skip"])
def test_restatement_against_reference(data, run):
    """integers and flags equal what the golden script recorded; floats within ten times the band it measured between the reference and
    this restatement when it ran (the band is a property of the reference's solver, not of any code under test)"""
    inp, golden = data
    tol = 10 * golden["measured_band"]
    assert 0 < tol < 1e-6
    rows = irep_ref.golden_rows(inp, golden["runs"][run])
    for g, row in zip(inp["genomes"], rows):
        acc = golden["runs"][run]["accessory"][g]
        for k in ("L", "num_contigs", "n_windows", "n_kept", "sum_cov", "flags"):
            assert row[k] == acc[k], (g, k, row[k], acc[k])
        if "iRep" in acc:
            mine = irep_ref.accessory(row)
            for k in irep_ref.GOLDEN_FLOATS + ("unfiltered_iRep",):
                assert irep_ref.rel_diff(mine[k], acc[k]) <= tol, (g, k, mine[k], acc[k])
            assert (acc["iRep"] is None) == np.isnan(row["irep"])
            if acc["iRep"] is not None:
                assert irep_ref.rel_diff(row["irep"], acc["iRep"]) <= tol
        else:
            assert np.isnan(row["irep"])


def _tables(inp, run, irep_rows):
    """GenomeTables of a golden run, fed with per-scaffold rows made in numpy from the stored coverage"""
    cov, mms = irep_ref.run_levels(inp, run)
    cum = np.cumsum(cov, axis=0)
    n_sc, M = len(inp["names"]), len(mms)
    lv = np.zeros((n_sc, M), dtype=_lib.SCAFFOLD_LEVEL_DT)
    for i in range(n_sc):
        s = slice(int(inp["bounds"][i]), int(inp["bounds"][i + 1]))
        lv["present"][i] = cov[:, s].any(axis=1)
        lv["nonzero"][i] = (cum[:, s] > 0).sum(axis=1)
        lv["sum_cov"][i] = cum[:, s].sum(axis=1)
        lv["mm"][i] = mms
    gt = gu.GenomeTables(inp["stb"], dict(zip(inp["names"], (int(x) for x in inp["lengths"]))))
    ids, genomes = gt.batch_genomes(inp["names"])
    acc, hist = genome_ref.coverage_rows_flat(cum, inp["bounds"], ids, len(genomes), mask_edges=100, hist_bins=None)
    gt.add_batch(inp["names"], inp["lengths"], lv, None, None, genomes, acc, hist, mms=mms)
    if irep_rows is not None:
        gt.set_irep(irep_ref.to_struct(irep_rows, _lib.IREP_ROW_DT))
    return gt


def assert_columns_equal(db, run, tol, skip):
    """the two iRep columns of a genome_info table against the reference's, row for row"""
    exp = {(r["genome"], r["mm"]): r for r in run["table"]}
    assert len(db) == len(exp)
    for _, r in db.iterrows():
        e = exp[(r["genome"], 1000 if skip else int(r["mm"]))]
        if e["iRep"] is None:
            assert np.isnan(r["iRep"]), (r["genome"], r["iRep"])
        else:
            assert irep_ref.rel_diff(r["iRep"], e["iRep"]) <= tol, (r["genome"], r["iRep"], e["iRep"])
        if e["iRep_GC_corrected"] is None:
            assert r["iRep_GC_corrected"] is not True and np.isnan(r["iRep_GC_corrected"]), (r["genome"], r["iRep_GC_corrected"])
        else:
            assert r["iRep_GC_corrected"] is e["iRep_GC_corrected"], (r["genome"], r["iRep_GC_corrected"])


@pytest.mark.parametrize("run", ["mm013", "mm02", "skip"])
def test_genome_tables_columns_against_reference(data, run):
    inp, golden = data
    r = golden["runs"][run]
    gt = _tables(inp, r, irep_ref.golden_rows(inp, r))
    assert gt.irep_level(irep_ref.run_levels(inp, r)[1], len(set(r["mm_of_level"])), r["skip_mm_profiling"]) == {"mm013": 1, "mm02": 0, "skip": 0}[run]
    db = gt.genome_info(skip_mm_profiling=r["skip_mm_profiling"])
    assert_columns_equal(db, r, 10 * golden["measured_band"], r["skip_mm_profiling"])
    if run != "mm02":
        assert db["iRep"].notna().sum() == (4 if run == "skip" else 12)
        acc = gt.irep_accessory()
        assert list(acc.columns) == ["genome", "kept_windows", "avg_cov", "r2", "fragMbp", "unfiltered_raw_iRep", "iRep_GC_corrected", "unfiltered_iRep"]
        assert list(acc["genome"]) == inp["genomes"]


def test_irep_level_mapping():
    gt = gu.GenomeTables({"a": "g"}, {"a": 300})
    assert gt.irep_level(None, 5) == 1 and gt.irep_level(None, 1) == 0 and gt.irep_level([0, 2, 7], 3) == 0
    assert gt.irep_level([2, 3], 2) == -1 and gt.irep_level([0, 1], 2) == 1 and gt.irep_level([1, 4], 2) == 0
    assert gt.irep_level([2, 3], 2, skip_mm_profiling=True) == 1


@pytest.mark.parametrize("run", ["mm013", "skip"])
def test_genome_tables_without_rows_gives_nan(data, run):
    inp, golden = data
    r = golden["runs"][run]
    db = _tables(inp, r, None).genome_info(skip_mm_profiling=r["skip_mm_profiling"])
    assert len(db) and db["iRep"].isna().all() and db["iRep_GC_corrected"].isna().all()
    assert db["iRep"].dtype == np.float64 and db["iRep_GC_corrected"].dtype == np.float64
