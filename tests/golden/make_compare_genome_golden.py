#!/usr/bin/env python3
"""tests/golden/make_compare_genome_golden.py -- golden vectors of the genome-level roll-up of `inStrain compare` tables.

Runs ONLY in the build container (needs the reference checkout): imports the reference's own inStrain.genomeUtilities under the stub
importer of make_golden.py and calls _add_stb (genomeUtilities.py:430-448) + _genome_wide_readComparer (:739-800) on a synthetic
comparisonsTable, with mm_level on and off.  Only data is stored: the input rows, the stb / bin2length and the reference's tables.

The input holds three samples (three pairs) over eight scaffolds of three genomes at mm levels {0, 1, 3}; scaffolds that miss a level
(the row of the level below then counts); a genome (gZ) whose compared_bases_count sums to 0 at every level (NaN columns); a scaffold
of gA with nothing compared at level 0 (NaN ANI on a row of a genome that has other rows); a scaffold the stb does not name.

usage: python tests/golden/make_compare_genome_golden.py
"""
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
import inStrain.genomeUtilities as gu                           # noqa: E402

rng = np.random.Generator(np.random.PCG64(909))
# name, genome (None: not in the stb), length, levels with a row
SCAFFOLDS = [("gA_1", "gA", 5200, (0, 1, 3)), ("gB_1", "gB", 1500, (0, 1, 3)), ("gA_2", "gA", 800, (1, 3)), ("gZ_1", "gZ", 400, (0, 1, 3)),
             ("gB_2", "gB", 2010, (0, 3)), ("free_1", None, 700, (0, 1, 3)), ("gA_3", "gA", 1301, (0, 1, 3)), ("gZ_2", "gZ", 90, (0,))]
SAMPLES = ["s1.bam", "s2.bam", "s3.bam"]
stb = {name: genome for name, genome, _, _ in SCAFFOLDS if genome is not None}
b2l = {}
for name, genome, ln, _ in SCAFFOLDS:
    if genome is not None:
        b2l[genome] = b2l.get(genome, 0) + ln

rows = []
for name, genome, ln, levels in SCAFFOLDS:
    for i in range(len(SAMPLES)):
        for j in range(i + 1, len(SAMPLES)):
            bases = 0
            for mm in levels:
                either = int(rng.integers(ln // 2, ln + 1))
                bases = min(either, bases + int(rng.integers(0, ln // 3 + 1)))
                if genome == "gZ" or (name == "gA_3" and mm == 0):
                    bases = 0
                snps = int(rng.integers(0, min(bases, 12) + 1))
                pop = int(rng.integers(0, snps + 1))
                rows.append({"mm": mm, "scaffold": name, "name1": SAMPLES[i], "name2": SAMPLES[j],
                             "coverage_overlap": bases / either if either > 0 else 0, "compared_bases_count": bases,
                             "percent_genome_compared": bases / ln, "length": ln, "consensus_SNPs": snps, "population_SNPs": pop,
                             "conANI": (bases - snps) / bases if bases else np.nan, "popANI": (bases - pop) / bases if bases else np.nan})
table = pd.DataFrame(rows).sample(frac=1.0, random_state=5).reset_index(drop=True)       # the reference sorts; the order must not matter
assert table[table["scaffold"] == "gA_3"]["conANI"].isna().any() and (table[table["scaffold"].str.startswith("gZ")]["compared_bases_count"] == 0).all()

table.to_csv(os.path.join(HERE, "compare_genome_table.csv"), index=False)
with open(os.path.join(HERE, "compare_genome_inputs.json"), "w") as f:
    json.dump({"stb": stb, "bin2length": b2l}, f, indent=1, sort_keys=True)
for mm_level, out in ((False, "compare_genome_golden.csv"), (True, "compare_genome_golden_mm.csv")):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = gu._genome_wide_readComparer(gu._add_stb(table, stb), stb, b2l, mm_level=mm_level)
    ref.to_csv(os.path.join(HERE, out), index=False)
    print(ref.to_string())
    print(ref.dtypes)
