#!/usr/bin/env python3
"""tests/golden/make_genome_info_golden.py -- golden vectors of the genome-level table (genome_info).

Runs ONLY in the build container (needs /root/reference): imports the reference's own
inStrain.genomeUtilities.genomeLevel_from_IS (genomeUtilities.py:145-269) under the stub importer of make_golden.py
(Bio / lmfit / pysam / h5py / seaborn are not installed: iRep fails inside its try and is not pinned) and calls it on a
duck-typed profile object, with and without skip_mm_profiling.  Only data is stored: the synthetic inputs and the
reference's tables.

The inputs hold three genomes interleaved over nine scaffolds; a scaffold present only at levels {1, 3} next to ones present at
{0, 1, 3}; a genome (gC) whose only scaffold first appears at the highest level; a scaffold with breadth_minCov == 0; rarefied
diversity missing on most rows; scaffolds of 150, 199 and 201 positions (the 2 x 100 masked edge positions); a scaffold the stb
names that has no length; one with a length that no read reached; one the stb does not name; LD rows whose (A, B) pair recurs at
two levels, LD rows with NaN r2 / d_prime and a genome without LD rows.

usage: python tests/golden/make_genome_info_golden.py
"""
import os
import sys
import warnings

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                                        # noqa: E402  (the stub importer)

mg.import_reference()
import inStrain.genomeUtilities as gu                           # noqa: E402

rng = np.random.Generator(np.random.PCG64(808))
LEVELS = (0, 1, 3)
# name, genome (None: not in the stb), length, levels with reads, depth of level 0
SCAFFOLDS = [("gA_1", "gA", 5200, (0, 1, 3), 14), ("gB_1", "gB", 150, (0, 1, 3), 12), ("gA_2", "gA", 199, (1, 3), 9),
             ("gB_2", "gB", 201, (0, 1, 3), 11), ("gC_1", "gC", 2600, (3,), 8), ("gB_3", "gB", 900, (0, 1), 2),
             ("gA_3", "gA", 1301, (0, 1, 3), 60), ("free_1", None, 700, (0, 1, 3), 10), ("gA_4", "gA", 640, (0, 3), 7)]
stb = {name: genome for name, genome, _, _, _ in SCAFFOLDS if genome is not None}
stb["gA_nolength"] = "gA"                                       # named by the stb, no length: counts in true_scaffolds only
stb["gB_noreads"] = "gB"                                        # has a length, no read: zeros in the coverage distribution
s2l = {name: ln for name, _, ln, _, _ in SCAFFOLDS}
s2l["gB_noreads"] = 400
b2l = {}
for sc, g in stb.items():                                       # prepare_genome_wide (:129-139)
    b2l.setdefault(g, 0)
    if sc in s2l:
        b2l[g] += s2l[sc]

MIN_COV, RARE_COV = 5, 50
covT, flat, raw, table = {}, [], [], []
for si, (name, genome, ln, levels, depth) in enumerate(SCAFFOLDS):
    covT[name] = {}
    cum = np.zeros(ln, dtype=np.int64)
    for mm in levels:
        frac = 0.85 if mm == levels[0] else 0.3
        k = np.sort(rng.choice(ln, size=max(int(ln * frac), 1), replace=False))
        hi = depth if mm == levels[0] else max(depth // 4, 2)
        v = rng.integers(max(hi // 2, 1), hi + 1, size=len(k)).astype("int32")
        covT[name][mm] = pd.Series(v, index=k.astype(np.int64))
        flat.append(np.c_[np.full(len(k), si), np.full(len(k), mm), k, v])
        cum[k] += v
        counted, rare = int((cum >= MIN_COV).sum()), int((cum >= RARE_COV).sum())
        sum_clon = float(rng.uniform(0.9, 1.0, size=counted).sum())
        sum_clon_r = float(rng.uniform(0.9, 1.0, size=rare).sum())
        div = int(rng.integers(0, 12))
        sns = int(rng.integers(0, div + 1))
        con = int(rng.integers(0, div + 1))
        pop = int(rng.integers(0, con + 1))
        raw.append((si, mm, int(np.count_nonzero(cum)), int(cum.sum()), counted, sum_clon, rare, sum_clon_r, div, sns, div - sns, con, pop))
        cov = cum.astype(np.float64)
        table.append({"scaffold": name, "length": ln, "breadth": np.count_nonzero(cum) / ln, "coverage": int(cum.sum()) / ln,
                      "coverage_median": int(np.median(cov)), "coverage_std": np.std(cov),
                      "coverage_SEM": np.std(cov, ddof=1) / np.sqrt(ln),
                      "nucl_diversity": 1 - sum_clon / counted if counted else np.nan,
                      "nucl_diversity_rarefied": 1 - sum_clon_r / rare if rare else np.nan,
                      "breadth_minCov": counted / ln, "breadth_rarefied": rare / ln,
                      "divergent_site_count": div, "SNS_count": sns, "SNV_count": div - sns, "consensus_divergent_sites": con,
                      "population_divergent_sites": pop,
                      "conANI_reference": (counted - con) / counted if counted else 0,
                      "popANI_reference": (counted - pop) / counted if counted else 0, "mm": mm})
sdb = pd.DataFrame(table)
assert (sdb[sdb["scaffold"] == "gB_3"]["breadth_minCov"] == 0).all() and sdb["nucl_diversity_rarefied"].isna().any()

ld = []
for name in ("gA_1", "gB_2", "gA_3", "free_1", "gA_4"):
    ln, levels = s2l[name], [x for x in SCAFFOLDS if x[0] == name][0][3]
    n_pairs = 3 if ln < 300 else 40
    a = np.sort(rng.choice(ln - 60, size=n_pairs, replace=False))
    for pa in a:
        pb = int(pa + rng.integers(1, 60))
        for mm in levels:
            if mm != levels[0] and rng.random() < 0.55:
                continue                                        # most pairs have one row; the others recur at a higher level
            r2 = float(rng.random()) if rng.random() > 0.15 else np.nan
            dp = float(rng.random()) if r2 == r2 and rng.random() > 0.1 else np.nan
            ld.append({"scaffold": name, "position_A": int(pa), "position_B": pb, "distance": pb - int(pa), "mm": mm, "r2": r2,
                       "d_prime": dp})
ldb = pd.DataFrame(ld)
assert ldb.duplicated(["scaffold", "position_A", "position_B"]).any() and ldb["r2"].isna().any() and ldb["d_prime"].isna().any()
mapping = pd.DataFrame({"scaffold": ["all_scaffolds"] + list(s2l), "filtered_pairs": np.arange(len(s2l) + 1)})


class Profile:
    """what genomeLevel_from_IS reads of an SNVprofile"""
    items = {"scaffold2bin": stb, "bin2length": b2l, "scaffold2length": s2l, "cumulative_scaffold_table": sdb, "mapping_info": mapping,
             "raw_linkage_table": ldb, "fasta_loc": None}

    def get(self, name, scaffolds=None, **kw):
        if name == "covT":
            return {s: c for s, c in covT.items() if scaffolds is None or s in scaffolds}
        v = self.items[name]
        return v.copy() if isinstance(v, pd.DataFrame) else v


DROP = ["iRep", "iRep_GC_corrected", "reads_filtered_pairs", "filtered_read_pair_count"]
for skip, out in ((False, "genome_info_golden.csv"), (True, "genome_info_golden_skipmm.csv")):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = gu.genomeLevel_from_IS(Profile(), skip_mm_profiling=skip)
    ref = ref[[c for c in ref.columns if c not in DROP and not c.startswith("reads_")]]
    ref.to_csv(os.path.join(HERE, out), index=False)
    print(ref.to_string())
    print(ref.dtypes)
sdb.to_csv(os.path.join(HERE, "genome_info_scaffold_table.csv"), index=False)
ldb.to_csv(os.path.join(HERE, "genome_info_linkage.csv"), index=False)
np.savez_compressed(
    os.path.join(HERE, "genome_info_inputs.npz"), scaffolds=np.array([x[0] for x in SCAFFOLDS]), lengths=np.array([x[2] for x in SCAFFOLDS]),
    stb=np.array(list(stb.items())), s2l_names=np.array(list(s2l)), s2l_lengths=np.array(list(s2l.values())), levels=np.array(LEVELS),
    cov=np.concatenate(flat).astype(np.int64),
    raw=np.array(raw, dtype=[("scaffold", "<i8"), ("mm", "<i8"), ("nonzero", "<i8"), ("sum_cov", "<i8"), ("counted", "<i8"), ("sum_clon", "<f8"),
                             ("counted_rarefied", "<i8"), ("sum_clon_rarefied", "<f8"), ("divergent", "<i8"), ("sns", "<i8"), ("snv", "<i8"),
                             ("con", "<i8"), ("pop", "<i8")]))
