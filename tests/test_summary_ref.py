"""Host: tests/summary_ref.py (the numpy reference the summary and compare edge tests hold the device against) is itself pinned --
against oracle/summary.py and oracle/compare.py, which the suite ties to the reference's golden vectors, and against the stored
merge_*_cumulative_scaffold_table.csv / compare_a .. compare_d fixtures where their columns map directly.  No GPU."""
import os

import numpy as np
import pandas as pd
import pytest

from tests import summary_ref as sr, util


def _observations(seed, bounds, M, depth=8, n_frac=0.02, skip=()):
    """reads as tests/test_gpu_rollup_edges.py::_reads makes them, bases 90 % reference, a few non-ACGT"""
    from tests.test_gpu_rollup_edges import _reads
    rng = np.random.Generator(np.random.PCG64(seed))
    gpos, mm, pair = _reads(rng, bounds, depth, M, skip=skip)
    codes = rng.integers(0, 4, int(bounds[-1])).astype(np.uint8)
    base = np.where(rng.random(len(gpos)) < 0.9, codes[gpos], rng.integers(0, 4, len(gpos))).astype(np.uint8)
    base[rng.random(len(gpos)) < n_frac] = 4
    return gpos, base, mm, pair, "".join(np.array(list("ACTG"))[codes])


@pytest.mark.parametrize("M", [1, 4])
def test_scaffold_levels_vs_oracle_coverage_table(M):
    """scaffolds of 300, 1, 599 and 200 positions (the last without reads): every column of oracle/summary.py coverage_table that maps
    onto a field, the covT keys against presence(), and the vectorised clonalities against the oracle's bit for bit"""
    from oracle import summary
    lut, fb = util.load_lut()
    bounds = np.array([0, 300, 301, 900, 1100], dtype=np.int64)
    gpos, base, mm, pair, seq = _observations(10 + M, bounds, M, skip=(3,))
    n_pos = int(bounds[-1])
    cov = sr.cov_levels(gpos, base, mm, n_pos, M)
    clon, results = sr.oracle_levels(bounds, gpos, base, mm, pair, seq, M, lut, fb)
    assert np.array_equal(clon, sr.clon_levels_from_counts(gpos, base, mm, n_pos, M), equal_nan=True)
    assert 0 < np.isnan(clon[-1, :900]).sum() < 900 and len(np.unique(clon[-1][~np.isnan(clon[-1])])) > 5
    present = sr.presence(gpos, base, mm, bounds, M)
    assert present[[0, 2]].all() and present[1].any() and not present[3].any()      # (the one-position scaffold may lack a level)
    # rarefied values: any per-entry numbers will do here, the same ones go to both sides
    rng = np.random.Generator(np.random.PCG64(99))
    clon_r = np.full((M, n_pos), np.nan)
    per_scaffold = []
    for i, r in enumerate(results):
        e = r["entries"]
        v = np.where(rng.random(len(e)) < 0.5, rng.random(len(e)), np.nan).astype(np.float32)
        per_scaffold.append(v)
        clon_r[:, int(bounds[i]):int(bounds[i + 1])] = sr.entry_levels(e["pos"], e["mm"], v, int(bounds[i + 1] - bounds[i]), M)
    got = sr.scaffold_levels(cov, clon, clon_r, present, bounds)
    for i, r in enumerate(results):
        L = int(bounds[i + 1] - bounds[i])
        rows = {row["mm"]: row for row in summary.coverage_table(r["entries"], r["snv"], L, clon_r=per_scaffold[i])}
        assert sorted(rows) == np.flatnonzero(got["present"][i]).tolist(), i
        for m, o in rows.items():
            g = {f: got[f][i, m] for f in sr.FIELDS}
            assert g["nonzero"] == round(o["breadth"] * L) and g["counted"] == round(o["breadth_minCov"] * L)
            assert g["counted_rarefied"] == round(o["breadth_rarefied"] * L)
            assert abs(g["sum_cov"] / L - o["coverage"]) < 1e-12 and int(g["median_cov"]) == o["coverage_median"]
            assert abs(np.sqrt(max(g["sumsq_cov"] / L - (g["sum_cov"] / L) ** 2, 0.0)) - o["coverage_std"]) < 1e-9
            for cnt, sm, med, col in (("counted", "sum_clon", "median_clon", "nucl_diversity"),
                                      ("counted_rarefied", "sum_clon_rarefied", "median_clon_rarefied", "nucl_diversity_rarefied")):
                if g[cnt]:
                    assert abs((1 - g[sm] / g[cnt]) - o[col]) < 1e-12 and 1 - g[med] == o[col + "_median"], (i, m, col)
                else:
                    assert np.isnan(g[med]) and np.isnan(o[col]) and np.isnan(o[col + "_median"]) and g[sm] == 0.0


@pytest.mark.parametrize("name", ["single", "triple", "double"])
def test_scaffold_levels_vs_stored_merge_tables(name):
    """the reference's own cumulative_scaffold_table of the merge fixtures (length, breadth, coverage, coverage_median, coverage_std,
    coverage_SEM, nucl_diversity, nucl_diversity_median, breadth_minCov per mm) and its stored clonT, from the fixtures' observations"""
    z = np.load(os.path.join(util.GOLD, "merge_inputs.npz"))
    names, lengths = [str(n) for n in z["names"]], z["lengths"].astype(np.int64)
    bounds = np.r_[0, np.cumsum(lengths)].astype(np.int64)
    i = names.index(name)
    s0, L = int(bounds[i]), int(lengths[i])
    k = (z["pos"] >= s0) & (z["pos"] < s0 + L)
    gpos, base, mm = z["pos"][k].astype(np.int64) - s0, z["base"][k], z["mm"][k].astype(np.int64)
    g = pd.read_csv(os.path.join(util.GOLD, "merge_%s_cumulative_scaffold_table.csv" % name))
    M = int(mm.max()) + 1
    cov = sr.cov_levels(gpos, base, mm, L, M)
    clon = sr.clon_levels_from_counts(gpos, base, mm, L, M)
    # the stored clonT: every stored (mm, position) value is the clonality of that level
    cm, cp, cv = z[name + "_clonT_mm"], z[name + "_clonT_pos"], z[name + "_clonT_val"]
    assert len(cv) > 1000 and (clon[cm, cp].astype(np.float32) == cv).all()
    got = sr.scaffold_levels(cov, clon, np.full((M, L), np.nan), sr.presence(gpos, base, mm, [0, L], M), [0, L])
    assert np.flatnonzero(got["present"][0]).tolist() == list(g["mm"]) and len(g) >= 3
    for _, o in g.iterrows():
        m = int(o["mm"])
        r = {f: got[f][0, m] for f in sr.FIELDS}
        assert o["length"] == L and r["nonzero"] / L == o["breadth"] and r["counted"] / L == o["breadth_minCov"]
        assert abs(r["sum_cov"] / L - o["coverage"]) < 1e-12 and int(r["median_cov"]) == o["coverage_median"]
        var = r["sumsq_cov"] / L - (r["sum_cov"] / L) ** 2
        assert abs(np.sqrt(var) - o["coverage_std"]) < 1e-9 and abs(np.sqrt(var * L / (L - 1)) / np.sqrt(L) - o["coverage_SEM"]) < 1e-9
        assert abs((1 - r["sum_clon"] / r["counted"]) - o["nucl_diversity"]) < 1e-12 and 1 - r["median_clon"] == o["nucl_diversity_median"]
        assert r["counted_rarefied"] == 0 and np.isnan(r["median_clon_rarefied"])


@pytest.mark.parametrize("levels", [(1, 4), (3, 6), (6, 3)])
def test_pair_levels_vs_oracle_compare(levels):
    """two samples with different numbers of levels on scaffolds of 300, 1, 599 and 200 positions (A has no read on the last, B none on
    the second): keys, compared bases and coverage_overlap of oracle/compare.py calc_mm2overlap + overlap_table at min_cov 1, 5 and 8"""
    from oracle import compare as ocompare, oracle
    lut, fb = util.load_lut()
    Ma, Mb = levels
    bounds = np.array([0, 300, 301, 900, 1100], dtype=np.int64)
    ga, ba, ma, pa, seq = _observations(21, bounds, Ma, depth=7, n_frac=0.0, skip=(3,))
    gb, bb, mb, pb, _ = _observations(22, bounds, Mb, depth=6, n_frac=0.0, skip=(1,))
    n_pos = int(bounds[-1])
    ca, cb = sr.cov_levels(ga, ba, ma, n_pos, Ma), sr.cov_levels(gb, bb, mb, n_pos, Mb)
    for min_cov in (1, 5, 8):
        pl = sr.pair_levels(ca, cb, sr.presence(ga, ba, ma, bounds, Ma), sr.presence(gb, bb, mb, bounds, Mb), bounds, min_cov)
        mm2overlap, mm2coverage = sr.overlap_dicts(pl)
        for i, (s0, s1) in enumerate(zip(bounds[:-1], bounds[1:])):
            def split(g, b, m, p):
                k = (g >= s0) & (g < s1)
                return oracle.profile_split(g[k] - s0, b[k], m[k], p[k], seq[s0:s1], 0, lut, fb)["entries"]
            o, c = ocompare.calc_mm2overlap(split(ga, ba, ma, pa), split(gb, bb, mb, pb), int(s1 - s0), min_cov=min_cov)
            assert sorted(o) == sorted(mm2overlap[i]) and (len(o) == max(Ma, Mb) or i in (1, 3)), (i, min_cov)
            assert {m: len(v) for m, v in o.items()} == mm2overlap[i] and c == mm2coverage[i], (i, min_cov)
            for t in ocompare.overlap_table(o, c, [], int(s1 - s0)):
                assert t["compared_bases_count"] == pl["both"][i, t["mm"]] and t["coverage_overlap"] == mm2coverage[i][t["mm"]]
        assert pl["both"][0, -1] > 0 and (pl["both"][3] == 0).all() and pl["either"][3, -1] > 0 and (pl["both"][1] == 0).all()


@pytest.mark.parametrize("name", ["compare_a", "compare_b", "compare_c", "compare_d"])
def test_pair_levels_vs_reference_vectors(name):
    """the reference's own calc_mm2overlap on the compare fixtures: levels, compared bases, coverage and the positions of the last level"""
    g = util.load_case(name)
    L = len(str(g["seq"]))
    Ma, Mb = int(g["a_mm"].max()) + 1, int(g["b_mm"].max()) + 1
    ca, cb = sr.cov_levels(g["a_pos"], g["a_base"], g["a_mm"], L, Ma), sr.cov_levels(g["b_pos"], g["b_base"], g["b_mm"], L, Mb)
    pl = sr.pair_levels(ca, cb, sr.presence(g["a_pos"], g["a_base"], g["a_mm"], [0, L], Ma),
                        sr.presence(g["b_pos"], g["b_base"], g["b_mm"], [0, L], Mb), [0, L], 5)
    o, c = sr.overlap_dicts(pl)
    assert sorted(o[0]) == list(g["mm"]) and [o[0][m] for m in g["mm"]] == list(g["both"])
    assert [c[0][m] for m in g["mm"]] == list(g["coverage"])
    assert np.flatnonzero((ca[-1] >= 5) & (cb[-1] >= 5)).tolist() == list(g["pos_in_both_last"])
