#!/usr/bin/env python3
"""tests/golden/make_mapping_info_golden.py -- golden vectors for the read report (build container only).

Writes mapping_info.bam (tests/bamwriter.py: five scaffolds -- three with messy pairs, one without a read, one with single
reads only -- plus hand-made pairs that fail exactly one criterion of evaluate_pair each, discordant pairs and single
priority reads) and runs the REFERENCE's own paired_read_filter + filter_scaff2pair2info (inStrain/filter_reads.py:471-532,
201-300; imported under the stub importer of make_golden.py) on the scaff2pair2info dictionaries that
oracle/bam_py.get_paired_reads builds from it, handed over in header order, for pairing_filter in {paired_only,
non_discordant, all_reads}, with and without priority reads.  Stores only data: the BAM, per case the whole Rdb
(mapping_info_<mode>_<p>.csv, %.17g floats), genomeUtilities._genome_wide_rr of it with the steps around it (:213-222;
..._genome.csv) and, in mapping_info.json, profile/fasta.py filter_fasta's kept scaffolds for a min_genome_coverage
between two genomes' estimates and for min_scaffold_reads alone."""
import json
import os
import sys
import tempfile

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

REFS = [("mA", 4000), ("mB", 3000), ("mEmpty", 2500), ("mSingle", 2000), ("mC", 3500)]
MESSY = [0, 1, 4]                       # the scaffolds random_reads fills
STB = {"mA": "gX", "mEmpty": "gX", "mB": "gY", "mC": "gZ"}         # mSingle: no genome
KW = dict(min_read_ani=0.93, min_mapq=1, max_insert_relative=3, min_insert=50)
MIN_SCAFFOLD_READS = 100


def _read(name, tid, pos, length, mate, mapq=40, nm=0):
    return dict(tid=tid, pos=pos, mapq=mapq, flag=0x1 | 0x2 | (0x40 if mate == 0 else 0x80), name=name, cigar=[("M", length)],
                seq="ACGT" * (length // 4) + "A" * (length % 4), qual=np.full(length, 37), nm=nm, isize=0, extra_tags=False)


def build_reads():
    from tests import bamwriter
    sub = [REFS[t] for t in MESSY]
    reads = bamwriter.random_reads(91, sub, 1500)
    for r in reads:
        r["tid"] = MESSY[r["tid"]]
    rng = np.random.Generator(np.random.PCG64(92))
    by_name = {}
    for r in reads:
        by_name.setdefault(r["name"], []).append(r)
    names = sorted(by_name, key=lambda n: int(n[1:]))
    # discordant pairs: the second read moves to another of the three scaffolds (a name on TWO scaffolds, never three)
    for n in rng.choice(names, 70, replace=False):
        rs = by_name[n]
        if len(rs) == 2:
            t = MESSY[(MESSY.index(rs[1]["tid"]) + 1 + int(rng.integers(0, 2))) % 3]
            rs[1]["tid"] = t
            rs[1]["pos"] = int(rng.integers(0, REFS[t][1] - 300))
    # a scaffold that holds single reads only
    singles = bamwriter.random_reads(93, [REFS[3]], 120)
    seen = set()
    for r in singles:
        if r["name"] in seen:
            continue
        seen.add(r["name"])
        r["name"] = "s" + r["name"][1:]
        r["tid"] = 3
        reads.append(r)
    # pairs that fail exactly one criterion (the others are comfortably met)
    for k in range(3):
        reads += [_read("ani%d" % k, 0, 500 + 10 * k, 60, 0, nm=9), _read("ani%d" % k, 0, 560 + 10 * k, 60, 1, nm=9)]
        reads += [_read("mq%d" % k, 1, 400 + 10 * k, 60, 0, mapq=0), _read("mq%d" % k, 1, 470 + 10 * k, 60, 1, mapq=1)]
        reads += [_read("lo%d" % k, 4, 300 + 10 * k, 30, 0), _read("lo%d" % k, 4, 305 + 10 * k, 30, 1)]
        reads += [_read("hi%d" % k, 0, 100 + 10 * k, 60, 0), _read("hi%d" % k, 0, 2900 + 10 * k, 60, 1)]
    reads.append(_read("odd0", 1, 900, 60, 0))
    reads.append(_read("odd0", 1, 980, 60, 1))
    reads.sort(key=lambda r: (r["tid"], r["pos"]))
    return reads


def main():
    import make_golden as mg
    mg.import_reference()
    import inStrain.filter_reads as fr
    import inStrain.genomeUtilities as gu
    import inStrain.profile.fasta as fa
    from oracle import bam_py
    from tests import bamwriter
    reads = build_reads()
    path = os.path.join(HERE, "mapping_info.bam")
    bamwriter.write_bam(path, REFS, reads)
    assert os.path.getsize(path) < 400_000, os.path.getsize(path)
    rrefs, rr = bam_py.read_bam(path)
    s2p2i = {}
    for t, (name, ln) in enumerate(rrefs):
        p2i = bam_py.get_paired_reads(rr, t)
        s2p2i[name] = {p: np.array(i, dtype="int64") for p, i in p2i.items()}
    assert len(s2p2i["mEmpty"]) == 0
    assert len(s2p2i["mSingle"]) > 50 and all(i[4] == 1 for i in s2p2i["mSingle"].values())
    n_entries = sum(len(d) for d in s2p2i.values())
    assert n_entries <= 2100, n_entries
    # priority reads: single reads of the messy scaffolds (never of mSingle: it stays without an entry under paired_only)
    single_names = sorted({p for s in ("mA", "mB", "mC") for p, i in s2p2i[s].items() if i[4] == 1}, key=lambda n: (len(n), n))
    priority = set(single_names[1::3])
    assert len(priority) >= 10
    with tempfile.TemporaryDirectory() as tmp:
        stb_loc = os.path.join(tmp, "golden.stb")
        with open(stb_loc, "w") as f:
            for s, g in STB.items():
                f.write("%s\t%s\n" % (s, g))
        stb = gu.load_scaff2bin([stb_loc])
        assert stb == STB
        s2l = dict(REFS)
        FAdb = pd.DataFrame({"scaffold": [n for n, _ in REFS], "start": 0, "end": [ln - 1 for _, ln in REFS], "split_number": 0})
        out = {"refs": REFS, "priority": sorted(priority), "params": KW, "stb": STB, "min_scaffold_reads": MIN_SCAFFOLD_READS, "cases": []}
        for mode in ("paired_only", "non_discordant", "all_reads"):
            for pr in (set(), priority):
                kw = dict(KW, pairing_filter=mode)
                tag = "%s_%d" % (mode, 1 if pr else 0)
                # the reference mutates the dictionaries (all_reads): hand it fresh copies, scaffolds in header order
                fresh = {s: {p: i.copy() for p, i in s2p2i[s].items()} for s, _ in REFS}
                tallys = {}
                try:
                    f = fr.paired_read_filter(fresh, priority_reads_set=pr, tallys=tallys, **kw)
                    s2p2mm, Rdb = fr.filter_scaff2pair2info(f, tallys, priority_reads_set=pr, **kw)
                except KeyError as e:
                    out["cases"].append({"mode": mode, "priority": bool(pr), "keyerror": True})
                    print(mode, bool(pr), "reference raised KeyError", e)
                    continue
                assert Rdb["scaffold"].tolist() == ["all_scaffolds"] + [n for n, _ in REFS]
                # ---- what the fixture is for, asserted on the reference's own output ----
                per = Rdb.iloc[1:].set_index("scaffold")
                median = float(np.median([v[1] for d in f.values() for v in d.values() if v[4] == 2]))
                alone = set()
                for d in f.values():
                    for v in d.values():
                        res = fr.evaluate_pair(v, np.zeros(4), kw["min_read_ani"], kw["min_mapq"], kw["min_insert"], median * 3)
                        if res.sum() == 3:
                            alone.add(int(np.flatnonzero(res == 0)[0]))
                assert alone == {0, 1, 2, 3}, alone                 # read ANI, max insert, min insert, mapq: each fails alone somewhere
                for c in Rdb.columns[1:13]:
                    if c.endswith("priority_reads") and not pr:
                        continue
                    if c == "filtered_singletons" and mode == "paired_only" and not pr:      # no single read gets that far
                        continue
                    assert per[c].sum() > 0, c                              # every counter moves ...
                    if c.startswith("pass_min") or c.startswith("pass_max") or c == "filtered_pairs":
                        assert (per[c] < per["pass_pairing_filter"]).any(), c   # ... and every criterion turns something down
                assert per.loc["mEmpty", "unfiltered_reads"] == 0 and np.isnan(per.loc["mEmpty", "median_insert"])
                assert per.loc["mSingle", "unfiltered_singletons"] > 50
                if mode == "paired_only":
                    assert per.loc["mSingle", "pass_pairing_filter"] == 0 and np.isnan(per.loc["mSingle", "mean_PID"])
                    assert int(Rdb.loc[0, "unfiltered_reads"]) == int(per.loc[["mA", "mB", "mC"], "unfiltered_reads"].sum())
                par = {int(per.loc[s, "pass_pairing_filter"]) % 2 for s in ("mA", "mB", "mC")}
                assert par == {0, 1}, per["pass_pairing_filter"].tolist()   # even and odd numbers of entries: both median branches
                if pr:
                    assert any(v[4] == 1 and v[1] == -1 and p in pr for d in f.values() for p, v in d.items())
                    assert per["filtered_priority_reads"].sum() > 0
                if mode == "all_reads":
                    assert any(v[1] == -2 for d in f.values() for v in d.values())
                # ---- genome level (genomeUtilities.py:213-222) ----
                rdb = Rdb[Rdb["scaffold"] != "all_scaffolds"]
                rdb = gu._add_stb(rdb, stb)
                rdb = gu._genome_wide_rr(rdb, stb)
                rdb = rdb.rename(columns={"reads_filtered_pairs": "filtered_read_pair_count"})
                if "reads_pass_pairing_filter" in rdb.columns:
                    del rdb["reads_pass_pairing_filter"]
                assert sorted(rdb["genome"]) == ["gX", "gY", "gZ"]
                # ---- filter_fasta (controller.py:265-271) ----
                s2p = Rdb.set_index("scaffold")["filtered_pairs"].to_dict()
                rl = float(Rdb.loc[0, "mean_pair_length"])
                est = {}
                for g in ("gX", "gY", "gZ"):
                    sc = [s for s, x in STB.items() if x == g]
                    est[g] = sum(s2p[s] for s in sc) * rl / sum(s2l[s] for s in sc)
                lo, mid = sorted(est.values())[:2]
                assert lo < mid
                thr = (lo + mid) / 2
                kept_cov = fa.filter_fasta(FAdb.copy(), s2p, s2l, rl, min_genome_coverage=thr, stb=[stb_loc])["scaffold"].tolist()
                kept_reads = fa.filter_fasta(FAdb.copy(), s2p, s2l, rl, min_scaffold_reads=MIN_SCAFFOLD_READS)["scaffold"].tolist()
                assert 0 < len(kept_cov) < 4 and 0 < len(kept_reads) < 5
                Rdb.to_csv(os.path.join(HERE, "mapping_info_%s.csv" % tag), index=False, float_format="%.17g")
                rdb.to_csv(os.path.join(HERE, "mapping_info_%s_genome.csv" % tag), index=False, float_format="%.17g")
                out["cases"].append({"mode": mode, "priority": bool(pr), "tag": tag, "dtypes": {c: str(t) for c, t in Rdb.dtypes.items()},
                                     "genome_dtypes": {c: str(t) for c, t in rdb.dtypes.items()},
                                     "median_insert": median, "readlength": rl, "genome_estimates": est, "min_genome_coverage": thr,
                                     "kept_min_genome_coverage": sorted(kept_cov, key=[n for n, _ in REFS].index),
                                     "kept_min_scaffold_reads": sorted(kept_reads, key=[n for n, _ in REFS].index)})
                print(tag, Rdb.iloc[0, 1:13].tolist(), "median", median, "estimates", est)
    json.dump(out, open(os.path.join(HERE, "mapping_info.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
