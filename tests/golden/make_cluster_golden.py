#!/usr/bin/env python3
"""tests/golden/make_cluster_golden.py -- golden vectors of strain clustering (`inStrain compare`'s strain_clusters.tsv).

Runs ONLY in the build container (needs the reference checkout and scipy): imports the reference's own inStrain.genomeUtilities and
inStrain.compare_utils under the stub importer of make_golden.py and runs, on a synthetic comparisonsTable,
    _add_stb + _genome_wide_readComparer (genomeUtilities.py:430-448, 739-800)  -> Mdb (genomeWide_compare)
    Mdb.sort_values + cluster_genome_strains (compare_controller.py:435-450, compare_utils.py:205-255) -> Cdb
for clusterAlg average / complete / weighted at ani_threshold 0.99999 and 0.999, and per genome the reference's own matrix
(add_av_RC, the pivot, squareform) with scipy's Z and labels.  Only data is stored.

The table: nine samples whose sorted order is not their order of insertion ("s10.bam" < "s2.bam"), mm levels {0, 1, 3} with the
highest one deciding, and the genomes
    gA_same     every sample, every distance 0
    gB_two      two clear strains, one of them with a sample 5e-5 away, and a sample below coverage_treshold (distance forced to 1)
    gC_chain    a-b 0, b-c 0, a-c above the cutoff: the order of the chain decides
    gD_zero     a pair with compared_bases_count 0: not clustered; sorted into the middle, so the cluster numbers skip it
    gE_pair     seen in two samples only
    gF_subset   five of the samples, three scaffolds, one of them with nothing compared for one pair (a NaN-ANI row)
and a scaffold the stb does not name.

The generator asserts what makes exact label equality a fair demand: all distances of a genome, its merge heights and both cutoffs are
pairwise either exactly equal or at least 1e-9 apart, and no genome has a missing pair.  It records the largest absolute difference
between the reference's distances / heights and those of the fp64 restatement (tests/cluster_ref.py), which sums a pair's rows in
scaffold order where the reference's order is whatever its unstable sort leaves.

usage: python tests/golden/make_cluster_golden.py
"""
import itertools
import json
import os
import sys
import warnings

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                                        # noqa: E402  (the stub importer)

mg.import_reference()
import inStrain.compare_utils as cu                             # noqa: E402
import inStrain.genomeUtilities as gu                           # noqa: E402
import scipy.cluster.hierarchy as sch                           # noqa: E402
import scipy.spatial.distance as ssd                            # noqa: E402

from tests import cluster_ref as cr                             # noqa: E402

rng = np.random.Generator(np.random.PCG64(1515))
SAMPLES = ["s2.bam", "s10.bam", "s1.bam", "s3.bam", "s11.bam", "s4.bam", "s5.bam", "s20.bam", "s6.bam"]      # order of insertion
assert sorted(SAMPLES) != SAMPLES
# name, genome (None: not in the stb), length -- in the order of the set, genomes interleaved
SCAFFOLDS = [("gB_1", "gB_two", 60000), ("gA_1", "gA_same", 50000), ("gF_1", "gF_subset", 30000), ("gD_1", "gD_zero", 20000),
             ("free_1", None, 7000), ("gC_1", "gC_chain", 100000), ("gF_2", "gF_subset", 45000), ("gA_2", "gA_same", 30000),
             ("gE_1", "gE_pair", 10000), ("gB_2", "gB_two", 40000), ("gF_3", "gF_subset", 5000), ("gD_2", "gD_zero", 9000)]
MEMBERS = {"gA_same": SAMPLES, "gB_two": ["s2.bam", "s10.bam", "s1.bam", "s3.bam", "s11.bam", "s4.bam"], "gC_chain": ["s5.bam", "s20.bam", "s6.bam"],
           "gD_zero": ["s2.bam", "s1.bam", "s3.bam"], "gE_pair": ["s10.bam", "s6.bam"], "gF_subset": ["s10.bam", "s1.bam", "s11.bam", "s5.bam", "s6.bam"],
           None: SAMPLES}
THRESHOLDS = (0.99999, 0.999)
COVERAGE_TRESHOLD = 0.1
stb = {name: genome for name, genome, _ in SCAFFOLDS if genome is not None}
b2l = {}
for name, genome, ln in SCAFFOLDS:
    if genome is not None:
        b2l[genome] = b2l.get(genome, 0) + ln


def top_row(name, genome, ln, a, b):
    """(compared bases, population SNPs) of the pair's highest-mm row on the scaffold"""
    both = int(0.8 * ln)
    if genome == "gA_same":
        return both, 0
    if genome == "gB_two":
        if "s4.bam" in (a, b):
            return int(0.02 * ln), 0                            # percent_compared 0.02 < coverage_treshold
        strain = {"s2.bam": 0, "s10.bam": 0, "s1.bam": 0, "s3.bam": 1, "s11.bam": 1}
        if strain[a] != strain[b]:
            return both, (100 + 3 * SAMPLES.index(a) + SAMPLES.index(b)) if name == "gB_1" else 60
        return both, 4 if ("s1.bam" in (a, b) and name == "gB_1") else 0
    if genome == "gC_chain":
        return both, 24 if {a, b} == {"s5.bam", "s6.bam"} else 0
    if genome == "gD_zero":
        return (0, 0) if {a, b} == {"s2.bam", "s3.bam"} else (both, 2)
    if genome == "gE_pair":
        return both, 1
    if genome == "gF_subset":
        if name == "gF_3" and {a, b} == {"s10.bam", "s1.bam"}:
            return 0, 0                                         # nothing compared: a NaN ANI on a row of a genome that has other rows
        return both - int(rng.integers(0, 500)), int(rng.integers(0, 40))
    return both, int(rng.integers(0, 10))


rows = []
for name, genome, ln in SCAFFOLDS:
    for a, b in itertools.combinations([s for s in SAMPLES if s in MEMBERS[genome]], 2):
        both, pop = top_row(name, genome, ln, a, b)
        levels = (0, 1, 3) if name != "gF_2" else (0, 3)
        for k, mm in enumerate(levels):
            last = k == len(levels) - 1
            bases = both if last else both * (k + 1) // 4
            p = pop if last else min(bases, pop + 7)            # lower levels would give other distances: only the last row may count
            snps = p + (1 if bases > p else 0)
            either = max(bases, int(0.9 * ln))
            rows.append({"mm": mm, "scaffold": name, "name1": a, "name2": b,
                         "coverage_overlap": bases / either if either > 0 else 0, "compared_bases_count": bases,
                         "percent_genome_compared": bases / ln, "length": ln, "consensus_SNPs": snps, "population_SNPs": p,
                         "conANI": (bases - snps) / bases if bases else np.nan, "popANI": (bases - p) / bases if bases else np.nan})
table = pd.DataFrame(rows).sample(frac=1.0, random_state=7).reset_index(drop=True)       # the reference sorts; the order must not matter

with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    Mdb = gu._genome_wide_readComparer(gu._add_stb(table, stb), stb, b2l, mm_level=False)
Mdb = Mdb.sort_values(["genome", "name1", "name2"]).reset_index(drop=True)

# the restatement from the same rows: its matrices, to compare and to check the fairness condition on
order = [name for name, _, _ in SCAFFOLDS]
pairs = cr.genome_pairs(table.to_dict("records"), stb, order)
mine = {g: cr.genome_matrix(p, b2l[g], COVERAGE_TRESHOLD) for g, p in pairs.items()}
assert all(st != cr.MISSING_PAIR for st, _, _ in mine.values())
assert [g for g, (st, _, _) in sorted(mine.items()) if st == cr.NO_OVERLAP] == ["gD_zero"]

golden = {"samples": SAMPLES, "scaffolds": [[n, ln] for n, _, ln in SCAFFOLDS], "stb": stb, "bin2length": b2l,
          "coverage_treshold": COVERAGE_TRESHOLD, "thresholds": list(THRESHOLDS), "genomes": {}, "cdb": {}}
worst = 0.0
for genome, gdb in Mdb.groupby("genome"):
    if not cu.evalute_genome_dist_matrix(gdb, genome):
        continue
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        adb = cu.add_av_RC(gdb, v2="percent_compared", n2="av_cov")
    adb["dist"] = 1 - adb["av_ani"]
    adb["dist"] = [1 if c < COVERAGE_TRESHOLD else d for d, c in zip(adb["dist"], adb["av_cov"])]
    db = adb.pivot(index="name1", columns="name2", values="dist")
    cond = ssd.squareform(np.asarray(db), checks=True)
    status, samples, m = mine[genome]
    assert status == cr.OK and list(db.columns) == samples
    my_cond = m[np.triu_indices(len(samples), 1)]
    worst = max(worst, float(np.abs(cond - my_cond).max()))
    entry = {"samples": samples, "condensed": cond.tolist(), "Z": {}, "labels": {}}
    for method in cr.METHODS:
        Z = sch.linkage(cond, method=method)
        myZ = cr.linkage(my_cond, len(samples), method)
        assert np.array_equal(Z[:, [0, 1, 3]], myZ[:, [0, 1, 3]])
        worst = max(worst, float(np.abs(Z[:, 2] - myZ[:, 2]).max()))
        assert cr.linkage(cond, len(samples), method).tobytes() == Z.tobytes()
        # the fairness condition: distances, heights and cutoffs pairwise equal or >= 1e-9 apart, for the reference's and our numbers
        for dist, heights in ((cond, Z[:, 2]), (my_cond, myZ[:, 2])):
            v = np.sort(np.r_[dist, heights, [1.0 - t for t in THRESHOLDS]])
            gap = np.diff(v)
            assert ((gap == 0) | (gap >= 1e-9)).all(), (genome, method, gap[(gap != 0) & (gap < 1e-9)])
        entry["Z"][method] = Z.tolist()
        entry["labels"][method] = {}
        for t in THRESHOLDS:
            lab = sch.fcluster(Z, 1 - t, criterion="distance")
            assert np.array_equal(lab, cr.fcluster(Z, len(samples), 1 - t))
            entry["labels"][method]["%r" % t] = lab.tolist()
    golden["genomes"][genome] = entry
for method in cr.METHODS:
    for t in THRESHOLDS:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            Cdb = cu.cluster_genome_strains(Mdb, {"clusterAlg": method, "ani_threshold": t, "coverage_treshold": COVERAGE_TRESHOLD})
        golden["cdb"]["%s %r" % (method, t)] = Cdb[["cluster", "sample", "genome"]].values.tolist()
golden["max_abs_diff"] = worst

table.to_csv(os.path.join(HERE, "cluster_table.csv"), index=False)
Mdb.to_csv(os.path.join(HERE, "cluster_mdb.csv"), index=False)
with open(os.path.join(HERE, "cluster_golden.json"), "w") as f:
    json.dump(golden, f, indent=1, sort_keys=True)
print(Mdb.to_string())
for k, v in golden["cdb"].items():
    print(k, sorted({(r[2], r[0]) for r in v}))
print("largest |reference - restatement| over distances and heights:", worst)
