"""GPU: profile_bam with the read report -- read_tables, the reads_* columns of genome_info, and the scaffold filters that read
the report (min_scaffold_reads, min_genome_coverage, database_mode)."""
import numpy as np
import pandas as pd
import pytest

import instrain_amd.profile as prof
from instrain_amd import engine
from instrain_amd.profile import filter_reads as fr
from instrain_amd.profile import profile_utilities as pu
from tests import bamwriter, util

pytestmark = pytest.mark.gpu

REFS = [("scafA", 2500), ("scafB", 700), ("scafC", 3100), ("scafD", 1500), ("scafE", 180), ("scafF", 2200)]
NAMES = [n for n, _ in REFS]
# g3 = scafF gets ten pairs (about half a fold of coverage) and they carry the run's highest mm; scafD is in no genome
STB = {"scafA": "g1", "scafC": "g1", "scafB": "g2", "scafE": "g2", "scafF": "g3"}
REMOVED = {"scafD", "scafF"}


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    lut, fb = util.load_lut()
    c.set_null_model(lut, fb)
    yield c
    c.close()


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("mapping_info")
    rng = np.random.Generator(np.random.PCG64(123))
    seqs = {n: "".join(rng.choice(list("ACGT"), ln)) for n, ln in REFS}
    reads = bamwriter.random_reads(31, REFS[:5], 5000)
    low = bamwriter.random_reads(32, [REFS[5]], 10)
    for r in low:
        r["tid"], r["name"], r["nm"], r["mapq"], r["flag"] = 5, "f" + r["name"][1:], 5, 40, r["flag"] & ~0x700
    reads = sorted(reads + low, key=lambda r: (r["tid"], r["pos"]))
    path = str(tmp / "report.bam")
    bamwriter.write_bam(path, REFS, reads)
    kept_path = str(tmp / "kept.bam")                # the same reads minus those of the scaffolds the genome filter removes
    bamwriter.write_bam(kept_path, REFS, [r for r in reads if NAMES[r["tid"]] not in REMOVED])
    lut, fb = util.load_lut()
    model = {int(i): int(v) for i, v in enumerate(lut) if v >= 0}
    model[-1] = fb
    return seqs, path, kept_path, model


def _kw(ctx, seqs, model, **more):
    kw = dict(s2s=seqs, null_model=model, min_cov=5, min_freq=0.05, min_snp=10, min_read_ani=0.9, window_length=1000, ctx=ctx,
              batch_positions=4000, strict=True)
    kw.update(more)
    return kw


def _same_splits(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        pd.testing.assert_frame_equal(a[k].raw_snp_table, b[k].raw_snp_table, check_exact=True)
        pd.testing.assert_frame_equal(a[k].raw_linkage_table, b[k].raw_linkage_table, check_exact=True)
        assert sorted(a[k].covT) == sorted(b[k].covT), k
        for mm in a[k].covT:
            assert (np.asarray(a[k].covT[mm]) == np.asarray(b[k].covT[mm])).all(), (k, mm)


@pytest.mark.parametrize("skip_mm", [False, True])
def test_read_tables_and_the_reads_columns_of_genome_info(ctx, case, skip_mm):
    seqs, path, _, model = case
    kw = _kw(ctx, seqs, model, skip_mm_profiling=skip_mm)
    st0, gt0 = {}, {}
    plain = prof.profile_bam(path, stb=STB, scaffold_tables=st0, genome_tables=gt0, **kw)
    st, gt, rt = {}, {}, {}
    splits = prof.profile_bam(path, stb=STB, scaffold_tables=st, genome_tables=gt, read_tables=rt, **kw)
    assert sorted(rt) == ["mapping_info", "scaffolds_removed"] and rt["scaffolds_removed"] == {}
    assert sorted(gt) == sorted(gt0) == ["bin2length", "genome_info", "scaffold2bin"]
    rdb = rt["mapping_info"]
    assert list(rdb.columns) == fr.COLUMNS and rdb["scaffold"].tolist() == ["all_scaffolds"] + NAMES
    assert int(rdb.loc[0, "filtered_pairs"]) > 3000
    rr = fr.genome_wide_rr(rdb, STB)
    got, base = gt["genome_info"], gt0["genome_info"]
    new = [c for c in got.columns if c not in base.columns]
    assert new == list(rr.columns[1:]) and "filtered_read_pair_count" in new and "reads_unfiltered_reads" in new
    # where the reference's merge puts them: after the coverage columns, before the four linkage columns
    assert sorted(got.columns[-4:]) == ["SNV_distance_mean", "d_prime_mean", "linked_SNV_count", "r2_mean"]
    assert list(got.columns[-4 - len(new):-4]) == new
    exp = pd.merge(got[["genome"]], rr, on="genome", how="left")
    pd.testing.assert_frame_equal(got[new].reset_index(drop=True), exp[new], check_exact=True)
    assert set(got["genome"]) >= {"g1", "g2"} and got[new].notna().all().all()
    pd.testing.assert_frame_equal(got[list(base.columns)], base, check_exact=True)
    _same_splits(splits, plain)
    assert sorted(st) == sorted(st0)
    for n in st:
        pd.testing.assert_frame_equal(st[n], st0[n], check_exact=True)


@pytest.mark.parametrize("skip_mm", [False, True])
def test_min_genome_coverage_equals_a_run_without_the_removed_reads(ctx, case, skip_mm):
    """run A lets the genome filter remove g3 (below 1x) and the scaffold in no genome; run C profiles a BAM without their reads,
    told the same filter set-up (all scaffolds exist for the filter, A's whole-file median): nothing of A exists only because of a
    removed scaffold -- not the highest mm level either, which only g3's pairs have"""
    seqs, path, kept_path, model = case
    kw = _kw(ctx, seqs, model, skip_mm_profiling=skip_mm)
    whole = engine.BamFile(path)
    whole.scan()
    info = whole.filter(min_read_ani=0.9)
    per_ref_mm = [max(whole.r2m(t).values(), default=0) for t in range(len(REFS))]
    whole.close()
    assert per_ref_mm[5] == 10 > max(per_ref_mm[:5])                 # the removed genome holds the pairs with the highest mm
    st_a, gt_a, rt_a, logs_a = {}, {}, {}, []
    a = prof.profile_bam(path, stb=STB, scaffold_tables=st_a, genome_tables=gt_a, read_tables=rt_a, min_genome_coverage=1, logs=logs_a, **kw)
    fdb = pd.DataFrame([(n, i, s, e) for n, ln in REFS if n not in REMOVED for i, (s, e) in enumerate(pu.iterate_splits(ln, 1000))],
                       columns=["scaffold", "split_number", "start", "end"])
    st_c, gt_c, rt_c = {}, {}, {}
    c = prof.profile_bam(kept_path, fdb, stb=STB, scaffold_tables=st_c, genome_tables=gt_c, read_tables=rt_c,
                         median_insert=info["median_insert"], filter_refs=list(range(len(REFS))), **kw)
    assert {k.rsplit(".", 1)[0] for k in a} == set(NAMES) - REMOVED
    _same_splits(a, c)
    if not skip_mm:
        assert max(max(S.covT, default=0) for S in a.values()) <= max(per_ref_mm[:5])
    pd.testing.assert_frame_equal(gt_a["genome_info"], gt_c["genome_info"], check_exact=True)
    assert set(gt_a["genome_info"]["genome"]) == {"g1", "g2"}
    assert sorted(st_a) == sorted(st_c) and not (set(st_a) & REMOVED)
    for n in st_a:
        pd.testing.assert_frame_equal(st_a[n], st_c[n], check_exact=True)
    assert rt_a["mapping_info"]["scaffold"].tolist() == ["all_scaffolds"] + NAMES          # made before anything was dropped
    assert set(rt_a["scaffolds_removed"]) == REMOVED
    assert "g3" in rt_a["scaffolds_removed"]["scafF"] and "1x" in rt_a["scaffolds_removed"]["scafF"]
    assert rt_a["scaffolds_removed"]["scafD"] == "no genome in the stb"
    assert not any(n in line for line in logs_a for n in REMOVED)


def test_database_mode_is_the_explicit_triple(ctx, case):
    seqs, path, _, model = case
    kw = _kw(ctx, seqs, model)
    del kw["min_read_ani"]
    gt_d, rt_d, gt_e, rt_e = {}, {}, {}, {}
    d = prof.profile_bam(path, stb=STB, genome_tables=gt_d, read_tables=rt_d, database_mode=True, **kw)
    e = prof.profile_bam(path, stb=STB, genome_tables=gt_e, read_tables=rt_e, min_read_ani=0.92, skip_mm_profiling=True,
                         min_genome_coverage=1, **kw)
    _same_splits(d, e)
    pd.testing.assert_frame_equal(rt_d["mapping_info"], rt_e["mapping_info"], check_exact=True)
    assert rt_d["scaffolds_removed"] == rt_e["scaffolds_removed"] and set(rt_d["scaffolds_removed"]) == REMOVED
    pd.testing.assert_frame_equal(gt_d["genome_info"], gt_e["genome_info"], check_exact=True)
    assert "mm" not in gt_d["genome_info"].columns and set(gt_d["genome_info"]["genome"]) == {"g1", "g2"}
    # and it differs from the plain run: the stricter read filter, the removed scaffolds
    plain = prof.profile_bam(path, **kw)
    assert {k.rsplit(".", 1)[0] for k in plain} - {k.rsplit(".", 1)[0] for k in d} >= {"scafD"}


def test_error_paths(ctx, case):
    seqs, path, _, model = case
    kw = _kw(ctx, seqs, model)
    with pytest.raises(ValueError):
        prof.profile_bam(path, min_genome_coverage=1, **kw)                   # no stb
    with pytest.raises(ValueError):
        prof.profile_bam(path, database_mode=True, **kw)                      # ... which database_mode asks for too
    whole = engine.BamFile(path)
    whole.scan()
    whole.filter(min_read_ani=0.9)
    r2m = {n: whole.r2m(t) for t, n in enumerate(NAMES)}
    whole.close()
    for bad in (dict(min_scaffold_reads=5), dict(min_genome_coverage=1, stb=STB), dict(database_mode=True, stb=STB)):
        with pytest.raises(ValueError):
            prof.profile_bam(path, None, r2m, **bad, **kw)
    rt = {}
    with_r2m = prof.profile_bam(path, None, r2m, read_tables=rt, **kw)
    assert rt == {} and len(with_r2m) > 0                                    # the controller's own read pairs: no filter ran here


def test_min_scaffold_reads_alone(ctx, case):
    seqs, path, _, model = case
    kw = _kw(ctx, seqs, model)
    rt, logs = {}, []
    got = prof.profile_bam(path, read_tables=rt, min_scaffold_reads=50, logs=logs, **kw)
    rdb = rt["mapping_info"].set_index("scaffold")
    few = {n for n in NAMES if rdb.loc[n, "filtered_pairs"] < 50}
    assert "scafF" in few and few != set(NAMES)
    assert set(rt["scaffolds_removed"]) == few and all("fewer than 50" in r for r in rt["scaffolds_removed"].values())
    assert {k.rsplit(".", 1)[0] for k in got} == set(NAMES) - few and logs == []
    plain = prof.profile_bam(path, **kw)
    for k in got:
        pd.testing.assert_frame_equal(got[k].raw_snp_table, plain[k].raw_snp_table, check_exact=True)
    # nothing is left: the empty dict and one error line
    rt, logs = {}, []
    assert prof.profile_bam(path, read_tables=rt, min_scaffold_reads=10 ** 6, logs=logs, **kw) == {}
    assert len(logs) == 1 and "No scaffolds passed initial filtering" in logs[0] and set(rt["scaffolds_removed"]) == set(NAMES)


SHARDED_WORKER = '''
import os, sys, json
sys.path.insert(0, %r)
import numpy as np
import torch
torch.cuda.set_device(0)
import torch.distributed as dist
from instrain_amd import dist as idist, engine
from instrain_amd.profile import filter_reads as fr
from tests import util
rank, local, world = idist.init_from_env(backend="gloo")
path, out = sys.argv[1], sys.argv[2]
z = np.load(sys.argv[3], allow_pickle=True)
seqs = {str(k): str(v) for k, v in zip(z["names"], z["seqs"])}
stb = json.loads(sys.argv[4])
lut, fb = util.load_lut()
model = {int(i): int(v) for i, v in enumerate(lut) if v >= 0}
model[-1] = fb
rt = {}
splits, tables, load = idist.profile_bam_sharded(path, seqs, model, rank, world, min_cov=5, min_freq=0.05, min_snp=10, min_read_ani=0.9,
                                                 window_length=1000, device=0, stb=stb, min_genome_coverage=1, read_tables=rt)
whole = engine.BamFile(path)
whole.scan(); whole.filter(min_read_ani=0.9)
exp = fr.mapping_info(whole.read_report(), [n for n, _, _ in whole.refs()])
assert rt["mapping_info"].equals(exp), rank                   # every rank holds the whole file's report
mine = sorted({S.scaffold for S in splits.values()})
every = [None] * world
dist.all_gather_object(every, (mine, sorted(rt["scaffolds_removed"])))
if rank == 0:
    assert tables["read_report"].equals(exp)
    json.dump({"scaffolds": [e[0] for e in every], "removed": [e[1] for e in every],
               "summary_tids": sorted(set(int(t) for t in tables["summary"]["tid"]))}, open(out, "w"))
else:
    assert tables is None
dist.barrier()
dist.destroy_process_group()
'''


def test_sharded_driver_filters_on_the_whole_files_report(case, tmp_path):
    """two ranks, each scanning its share of the BAM: the report both hold is the whole file's, the genome filter removes the same
    scaffolds on both before they are dealt, and rank 0 returns the table as `read_report`"""
    import json
    import os
    import sys
    seqs, path, _, _ = case
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    np.savez(str(tmp_path / "seqs.npz"), names=np.array(list(seqs)), seqs=np.array(list(seqs.values())))
    script = tmp_path / "w.py"
    script.write_text(SHARDED_WORKER % repo)
    out = str(tmp_path / "out.json")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29579")
    r = util.run_group([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29579", str(script), path, out, str(tmp_path / "seqs.npz"),
                        json.dumps(STB)], env=env, timeout=240)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    g = json.load(open(out))
    assert all(set(rm) == REMOVED for rm in g["removed"])
    assert sorted(s for sc in g["scaffolds"] for s in sc) == sorted(set(NAMES) - REMOVED)
    assert g["summary_tids"] == [t for t, n in enumerate(NAMES) if n not in REMOVED]
