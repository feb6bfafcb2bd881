"""The read report (host only): isx_bam_read_report / isx_bam_drop_refs, profile.filter_reads.* against what the REFERENCE's
own filter_scaff2pair2info, _genome_wide_rr and filter_fasta made of tests/golden/mapping_info.bam
(tests/golden/make_mapping_info_golden.py)."""
import io
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pandas as pd
import pytest

from instrain_amd import _lib, engine
from instrain_amd.profile import filter_reads as fr
from tests import bamwriter, util

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = json.load(open(os.path.join(util.GOLD, "mapping_info.json")))
BAM = os.path.join(util.GOLD, "mapping_info.bam")
NAMES = [n for n, _ in G["refs"]]
CASES = [c for c in G["cases"] if not c.get("keyerror")]
EXACT = fr.COUNT_COLUMNS + [c for c, _ in fr.MEAN_COLUMNS] + ["median_insert"]
EPS = 2.0 ** -52


def _report(case, threads=0, wanted=None):
    bam = engine.BamFile(BAM, threads=threads)
    bam.scan()
    if case["priority"]:
        bam.set_priority_reads(G["priority"])
    bam.set_wanted_refs(wanted)
    bam.filter(pairing_filter=case["mode"], **G["params"])
    return bam, bam.read_report()


def _same(a, b):
    """exactly equal, NaN where NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def _csv_round_trip(db):
    return pd.read_csv(io.StringIO(db.to_csv(index=False, float_format="%.17g")), float_precision="round_trip")


def _check_pid(got, exp, n_terms, what):
    """sum of n same-sign doubles in another order than numpy's pairwise sum: n * 2^-52 relative at worst"""
    got, exp, n_terms = np.asarray(got, np.float64), np.asarray(exp, np.float64), np.asarray(n_terms, np.float64)
    assert (np.isnan(got) == np.isnan(exp)).all(), what
    ok = ~np.isnan(exp)
    assert (np.abs(got[ok] - exp[ok]) <= n_terms[ok] * EPS * np.abs(exp[ok])).all(), (what, got, exp)


def test_the_golden_covers_every_case():
    assert len(G["cases"]) == 6 and len(CASES) == 6
    assert {(c["mode"], c["priority"]) for c in CASES} == {(m, p) for m in ("paired_only", "non_discordant", "all_reads") for p in (False, True)}


@pytest.mark.parametrize("case", CASES, ids=[c["tag"] for c in CASES])
def test_mapping_info_matches_the_reference(case):
    bam, rows = _report(case)
    got = fr.mapping_info(rows, NAMES)
    exp = pd.read_csv(os.path.join(util.GOLD, "mapping_info_%s.csv" % case["tag"]), float_precision="round_trip")
    assert list(got.columns) == list(exp.columns) == fr.COLUMNS
    assert got["scaffold"].tolist() == exp["scaffold"].tolist() == ["all_scaffolds"] + NAMES
    assert {c: str(t) for c, t in got.dtypes.items()} == case["dtypes"]            # as the reference held it in memory
    assert (_csv_round_trip(got).dtypes == exp.dtypes).all()                        # ... and as it reads back from the CSV
    for c in EXACT:
        assert _same(got[c], exp[c]), (c, got[c].tolist(), exp[c].tolist())
    n = exp["pass_pairing_filter"].values.astype(np.float64)
    n[0] = n[1:].max()                              # all_scaffolds: the largest bound of its rows
    _check_pid(got["mean_PID"], exp["mean_PID"], n, "mean_PID")
    bam.close()


@pytest.mark.parametrize("case", CASES, ids=[c["tag"] for c in CASES])
def test_genome_wide_rr_and_filter_scaffolds_match_the_reference(case):
    bam, rows = _report(case)
    bam.close()
    rdb = fr.mapping_info(rows, NAMES)
    got = fr.genome_wide_rr(rdb, G["stb"])
    exp = pd.read_csv(os.path.join(util.GOLD, "mapping_info_%s_genome.csv" % case["tag"]), float_precision="round_trip")
    assert list(got.columns) == list(exp.columns) and got["genome"].tolist() == exp["genome"].tolist()
    assert "filtered_read_pair_count" in got.columns and "reads_pass_pairing_filter" not in got.columns
    assert {c: str(t) for c, t in got.dtypes.items()} == case["genome_dtypes"]
    assert (_csv_round_trip(got).dtypes == exp.dtypes).all()
    per = rdb.iloc[1:].copy()
    per["genome"] = per["scaffold"].map(G["stb"])
    n = per.groupby("genome")["pass_pairing_filter"].max().reindex(exp["genome"]).values
    for c in exp.columns[1:]:
        if c == "reads_mean_PID":
            _check_pid(got[c], exp[c], n, c)
        else:
            assert _same(got[c], exp[c]), (c, got[c].tolist(), exp[c].tolist())
    s2p = rdb.set_index("scaffold")["filtered_pairs"].to_dict()
    s2l = dict(G["refs"])
    rl = float(rdb.loc[0, "mean_pair_length"])
    assert rl == case["readlength"]
    kept, removed = fr.filter_scaffolds(NAMES, s2p, s2l, rl, min_genome_coverage=case["min_genome_coverage"], stb=G["stb"])
    assert kept == case["kept_min_genome_coverage"] and sorted(kept + list(removed)) == sorted(NAMES)
    assert removed["mSingle"] == "no genome in the stb" and "coverage" in removed["mA"] and "coverage" in removed["mEmpty"]
    kept, removed = fr.filter_scaffolds(NAMES, s2p, s2l, rl, min_scaffold_reads=G["min_scaffold_reads"])
    assert kept == case["kept_min_scaffold_reads"] and sorted(kept + list(removed)) == sorted(NAMES)
    assert all("fewer than" in r for r in removed.values())
    assert fr.filter_scaffolds(NAMES, s2p, s2l, rl) == (NAMES, {})
    with pytest.raises(ValueError):
        fr.filter_scaffolds(NAMES, s2p, s2l, rl, min_genome_coverage=1)


def test_filter_scaffolds_logs_the_reference_lines(caplog):
    import logging
    s2p = {"a": 100, "b": 1, "c": 5}
    with caplog.at_level(logging.INFO):
        kept, removed = fr.filter_scaffolds(["a", "b", "c"], s2p, {"a": 1000, "b": 1000, "c": 10}, 100.0, min_genome_coverage=1,
                                            stb={"a": "g1", "b": "g2"})
    assert kept == ["a"] and set(removed) == {"b", "c"}
    assert "1 of 2 genomes have less than 1x estimated coverage" in caplog.text
    assert "2 of the original 3 scaffolds are removed (1 have a low coverage genome; 1 have no genome)" in caplog.text


@pytest.mark.parametrize("case", [CASES[1], CASES[5]], ids=lambda c: c["tag"])
def test_rows_do_not_depend_on_the_thread_count(case):
    b1, r1 = _report(case, threads=1)
    b16, r16 = _report(case, threads=16)
    assert r1.dtype == _lib.READ_REPORT_DT and r1.tobytes() == r16.tobytes()
    b1.close(); b16.close()


def test_blocks_inside_a_reference_do_not_depend_on_the_thread_count(tmp_path):
    """one reference of more entries than a piece of the sweep holds (65536): the pieces' partial sums are put together the same way
    on any number of threads"""
    rng = np.random.Generator(np.random.PCG64(5))
    n = 70000
    pos = np.sort(rng.integers(0, 50000, n))
    reads = []
    for i in range(n):
        for mate in (0, 1):
            reads.append(dict(tid=0, pos=int(pos[i]) + 40 * mate, mapq=int(rng.integers(0, 40)), flag=0x1 | 0x2 | (0x40 if mate == 0 else 0x80),
                              name="q%d" % i, cigar=[("M", 20)], seq="ACGTACGTACGTACGTACGT", qual=np.full(20, 37), nm=int(rng.integers(0, 3)),
                              isize=0, extra_tags=False))
    reads.sort(key=lambda r: r["pos"])
    path = str(tmp_path / "big.bam")
    bamwriter.write_bam(path, [("big", 51000)], reads)
    out = []
    for threads in (1, 16):
        bam = engine.BamFile(path, threads=threads)
        bam.scan()
        bam.filter(min_mapq=5)
        out.append(bam.read_report())
        bam.close()
    assert out[0]["pass_pairing_filter"][0] == n and 0 < out[0]["pass_min_mapq"][0] < n
    assert out[0].tobytes() == out[1].tobytes()


def test_unwanted_references_get_zero_rows():
    case = CASES[0]
    bam, rows = _report(case, wanted=[1, 4])
    whole, all_rows = _report(case)
    zero = np.zeros(1, dtype=_lib.READ_REPORT_DT)
    zero["median_insert"] = np.nan
    for t in (0, 2, 3):
        assert rows[t:t + 1].tobytes() == zero.tobytes()
    # only the whole-file median (the max insert) ties the scaffolds together under paired_only
    for t in (1, 4):
        for f in ("unfiltered_reads", "pass_pairing_filter", "pass_min_read_ani", "pass_min_mapq", "sum_mismatches", "median_insert"):
            assert rows[f][t] == all_rows[f][t]
    got = fr.mapping_info(rows, NAMES, wanted=[4, 1])
    assert got["scaffold"].tolist() == ["all_scaffolds", "mB", "mC"]
    bam.close(); whole.close()


def test_report_needs_a_filter_run():
    bam = engine.BamFile(BAM)
    with pytest.raises(engine.IsxError) as e:
        bam.read_report()
    assert e.value.code == -6                       # ISX_ERR_STATE
    bam.scan()
    with pytest.raises(engine.IsxError) as e:
        bam.read_report()
    assert e.value.code == -6 and "isx_bam_filter first" in str(e.value)
    bam.close()


def test_report_is_unchanged_by_drop_names_and_drop_refs():
    bam, rows = _report(CASES[3])
    before = rows.tobytes()
    bam.drop_names()
    assert bam.read_report().tobytes() == before
    bam.drop_refs([0, 3])
    assert bam.read_report().tobytes() == before
    bam.close()


def test_drop_refs_leaves_what_a_filter_without_those_pairs_leaves(tmp_path):
    """handle A drops two references after the filter; on BAM B every read of those references has mapq 0, so the same filter
    lets none of their pairs through (inserts, names and everything else are the same: the same median): totals, per-reference
    counts and mm levels agree.  The highest mm sits on a dropped reference."""
    refs = [("d%d" % i, 3000) for i in range(4)]
    reads = bamwriter.random_reads(17, refs, 1200)
    for r in reads:
        r["mapq"] = max(r["mapq"], 3)
        if r["tid"] == 2 and r["nm"] == 3:
            r["nm"] = 7                              # levels 7 .. 14 exist on d2 only
    pa, pb = str(tmp_path / "a.bam"), str(tmp_path / "b.bam")
    bamwriter.write_bam(pa, refs, reads)
    for r in reads:
        if r["tid"] in (0, 2):
            r["mapq"] = 0
    bamwriter.write_bam(pb, refs, reads)
    kw = dict(min_read_ani=0.8, min_mapq=1)
    a, b = engine.BamFile(pa), engine.BamFile(pb)
    for h in (a, b):
        h.scan()
        h.filter(**kw)
    levels_before = a.mm_levels()
    assert a.info["filtered_pairs"] > b.info["filtered_pairs"] > 0 and a.info["max_mm"] > b.info["max_mm"]
    info = a.drop_refs([0, 2])
    assert info == a.info == b.info
    for x, y in zip(a.ref_counts(), b.ref_counts()):
        assert (x == y).all()
    assert a.ref_counts()[1][0] == 0 and a.ref_counts()[1][2] == 0 and a.ref_counts()[1][1] > 0
    assert (a.mm_levels() == b.mm_levels()).all() and len(a.mm_levels()) < len(levels_before)
    assert a.r2m(0) == {} and a.r2m(1) == b.r2m(1) and a.r2m(3) == b.r2m(3)
    with pytest.raises(engine.IsxError):
        a.drop_refs([4])
    a.close(); b.close()


def test_write_mapping_info_round_trip(tmp_path):
    case = CASES[2]
    bam, rows = _report(case)
    bam.close()
    rr = fr.mapping_info(rows, NAMES)
    loc = str(tmp_path / "mapping_info.tsv")
    open(loc, "w").write("stale\n")
    kw = dict(G["params"], pairing_filter=case["mode"])
    values = fr.write_mapping_info(rr, loc, **kw)
    assert values == fr.write_mapping_info(rr, None, **kw)
    first = open(loc).readline()
    assert first == "# min_read_ani:0.93 max_insert_relative:3 min_insert:50 min_mapq:1 pairing_filter:non_discordant\n"
    back = pd.read_csv(loc, sep="\t", comment="#", float_precision="round_trip")
    pd.testing.assert_frame_equal(back, rr, check_exact=True)       # values and dtypes: no digit is lost in the file
    assert list(back.columns) == fr.COLUMNS and back["scaffold"].tolist() == rr["scaffold"].tolist()


def test_filter_reads_runs_without_a_context(monkeypatch):
    def no_context(*a, **k):
        raise AssertionError("filter_reads must not open a device context")
    monkeypatch.setattr(engine, "Context", no_context)
    case = CASES[1]
    rr = fr.filter_reads(BAM, priority_reads=G["priority"], pairing_filter=case["mode"], **G["params"])
    bam, rows = _report(case)
    bam.close()
    pd.testing.assert_frame_equal(rr, fr.mapping_info(rows, NAMES), check_exact=True)
    sub = fr.filter_reads(BAM, scaffolds=["mC", "mB", "nowhere"], **G["params"])
    assert sub["scaffold"].tolist() == ["all_scaffolds", "mB", "mC"]
    with pytest.raises(ValueError):                 # no name matches: not "every reference"
        fr.filter_reads(BAM, scaffolds=["nowhere"], **G["params"])


def test_genome_wide_rr_on_many_scaffolds_with_gaps():
    """genomes of 1 .. 40 scaffolds in shuffled order, scaffolds without an entry (NaN means) and without a genome, one genome whose
    scaffolds are all empty: sums exact and dtype-preserving, means = the mean of the scaffolds that have a value"""
    rng = np.random.Generator(np.random.PCG64(9))
    n = 300
    rows = np.zeros(n, dtype=_lib.READ_REPORT_DT)
    for f in _lib.READ_REPORT_DT.names[:16]:
        rows[f] = rng.integers(0, 5000, n)
    rows["pass_pairing_filter"] = rng.integers(1, 3000, n)
    rows["sum_pid"] = rng.random(n) * rows["pass_pairing_filter"]
    rows["median_insert"] = rng.integers(50, 400, n) / 2.0
    empty = rng.random(n) < 0.2
    names = ["c%d" % i for i in range(n)]
    sizes = [1, 2, 7, 8, 9, 40, 33, 3]
    gen = np.repeat(np.arange(len(sizes)), sizes)
    stb = {names[i]: "G%02d" % g for i, g in zip(rng.permutation(n)[:len(gen)], gen)}
    empty |= np.array([stb.get(nm) == "G07" for nm in names])
    rows["pass_pairing_filter"][empty] = 0
    rows["median_insert"][empty] = np.nan
    rdb = fr.mapping_info(rows, names)
    got = fr.genome_wide_rr(rdb, stb)
    per = rdb.iloc[1:].copy()
    per["genome"] = per["scaffold"].map(stb)
    grp = per[per["genome"].notna()].groupby("genome")
    assert got["genome"].tolist() == sorted(set(stb.values())) and len(got) == len(sizes)
    for c in fr.COLUMNS[1:]:
        if c == "pass_pairing_filter":
            assert "reads_" + c not in got.columns
            continue
        col = "filtered_read_pair_count" if c == "filtered_pairs" else "reads_" + c
        if c in fr.COUNT_COLUMNS:
            assert got[col].dtype == rdb[c].dtype and (got[col].values == grp[c].sum().values).all(), c
        else:
            exp = np.array([np.mean(x.dropna().values) if x.notna().any() else np.nan for _, x in grp[c]])
            assert _same(got[col], exp), c
            assert np.isnan(got[col].values[-1]) and not np.isnan(got[col].values[2:-1]).any()       # G07 is all empty
    assert list(got.columns[1:]) == [("filtered_read_pair_count" if c == "filtered_pairs" else "reads_" + c) for c in fr.COLUMNS[1:]
                                     if c != "pass_pairing_filter"]


def test_sars_read_report_integer_columns():
    """the stored report was written by an older release whose all_scaffolds row follows another rule: only the per-scaffold
    integer columns both share"""
    exp = pd.read_csv(os.path.join(util.GOLD, "sars_cov_2_read_report.csv.gz"), comment="#")
    exp = exp[exp["scaffold"] == "MT039887.1"].iloc[0]
    got = fr.filter_reads(os.path.join(util.GOLD, "sars_cov_2.sorted.bam"))
    got = got[got["scaffold"] == "MT039887.1"].iloc[0]
    for c in ("unfiltered_reads", "unfiltered_pairs", "unfiltered_singletons", "unfiltered_priority_reads", "pass_pairing_filter",
              "pass_max_insert", "pass_min_insert", "pass_min_mapq", "filtered_pairs", "filtered_singletons", "filtered_priority_reads"):
        assert int(got[c]) == int(exp[c]), c


REPORT_WORKER = textwrap.dedent("""
    import os, sys
    sys.path.insert(0, %r)
    import numpy as np
    import torch.distributed as dist
    from instrain_amd import dist as idist, engine
    from instrain_amd.profile import filter_reads as fr
    rank, local, world = idist.init_from_env(backend="gloo")
    path = sys.argv[1]
    for mode in ("paired_only", "non_discordant"):
        fkw = dict(pairing_filter=mode, min_read_ani=0.9)
        bam = engine.BamFile(path, threads=2)
        names = [n for n, _, _ in bam.refs()]
        bam.scan(part=(rank, world))
        if mode == "paired_only":
            ins = idist.all_gather_concat(bam.insert_sizes())
        else:
            idist.resolve_cross_names(bam, rank, world)
            bam.filter(median_insert=0.0, **fkw)
            ins = idist.all_gather_concat(bam.filter_insert_sizes())
        bam.filter(median_insert=float(np.median(ins)), **fkw)
        rows = idist.gather_read_report(bam, sharded=True)
        got = fr.mapping_info(rows, names)
        whole = engine.BamFile(path, threads=2)
        whole.scan()
        whole.filter(**fkw)
        w_rows = whole.read_report()
        assert rows.tobytes() == w_rows.tobytes(), (rank, rows, w_rows)
        assert got.equals(fr.mapping_info(w_rows, names)) and int(got.loc[0, "filtered_pairs"]) > 1000
        own = bam.read_report()["unfiltered_reads"] > 0
        assert 0 < own.sum() < (w_rows["unfiltered_reads"] > 0).sum()            # a share holds some of the rows, not all
        if rank == 0:
            print("REPORT_OK", mode, world, int(own.sum()))
    dist.barrier()
    dist.destroy_process_group()
""") % REPO


@pytest.mark.parametrize("world,port", [(2, 29561), (3, 29562)])
def test_gathered_read_report_of_the_shares(tmp_path, world, port):
    """every rank scans its share, the rows of the references it owns are all-gathered: the same bytes as one handle over the
    whole file, on every rank -- for paired_only and for non_discordant (names resolved across the shares)"""
    path = str(tmp_path / "cross.bam")
    bamwriter.cross_scaffold_bam(path, 71, triple=False)
    script = tmp_path / "report_worker.py"
    script.write_text(REPORT_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
                        "--master-addr", "127.0.0.1", "--master-port", str(port), str(script), path],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    for mode in ("paired_only", "non_discordant"):
        assert "REPORT_OK %s %d" % (mode, world) in r.stdout


def test_sharded_driver_hands_the_finished_report_on_and_leaves_the_plain_call_alone(monkeypatch):
    """profile_bam_sharded up to its profile_bam call (stubbed: no device here): with the keywords the handle arrives filtered, with the
    removed scaffolds dropped, next to the finished table; without them none of the report's steps runs"""
    from instrain_amd import dist as idist
    from instrain_amd.profile import profile_utilities as pu
    seqs = {n: "A" * ln for n, ln in G["refs"]}
    seen = {}

    def stub(bam, fdb, *a, **k):
        seen.update(scaffolds=sorted(set(fdb["scaffold"])), done=k.get("read_report_done"), pairs=k["bamfile"].ref_counts()[1].copy())
        return {}
    monkeypatch.setattr(pu, "profile_bam", stub)
    calls = []
    for name in ("read_report", "drop_refs"):
        real = getattr(engine.BamFile, name)
        monkeypatch.setattr(engine.BamFile, name, lambda self, *a, _n=name, _r=real: (calls.append(_n), _r(self, *a))[1])
    case = CASES[0]
    rt = {}
    _, tables, _ = idist.profile_bam_sharded(BAM, seqs, {}, 0, 1, stb=G["stb"], min_genome_coverage=case["min_genome_coverage"],
                                             read_tables=rt, **G["params"])
    rdb, removed = seen["done"]
    assert seen["scaffolds"] == sorted(case["kept_min_genome_coverage"]) and set(removed) == set(NAMES) - set(seen["scaffolds"])
    assert tables["read_report"] is rdb and rt["mapping_info"] is rdb and rt["scaffolds_removed"] == removed
    assert all(seen["pairs"][NAMES.index(n)] == 0 for n in removed) and seen["pairs"].sum() > 0
    assert calls == ["read_report", "drop_refs"]
    del calls[:]
    _, tables, _ = idist.profile_bam_sharded(BAM, seqs, {}, 0, 1, **G["params"])
    assert calls == [] and seen["done"] is None and "read_report" not in tables and seen["scaffolds"] == sorted(NAMES)
