#!/usr/bin/env python3
"""tests/golden/make_pool_golden.py -- golden vectors of SNV pooling across samples (`inStrain compare --bams`).

Runs ONLY in the build container (needs the reference checkout): imports the reference's own inStrain.polymorpher under the stub
importer of make_golden.py.  Four samples over six scaffolds (lengths 1, 63, 64, 65, 129, 300) at min_cov 5:
  observations -> make_golden.run_reference_split per (sample, scaffold) -> the reference's SNV tables (mm, cryptic)
  PoolController.__init__ on duck-typed profiles -> its own rows; extract_SNV_positions -> sites and what every sample pulls
  get_pooling_counts on make_golden.columns_from_obs columns -> the pulled counts (the BAM pile-up stands behind those columns)
  genreate_pooled_SNV_table / generate_pooled_SNV_summary_table -> DSTdb / PMdb
Only data is stored: the observations (pool_obs.npz) and the reference's two tables (pool_DSTdb.csv, pool_PMdb.csv).

What the inputs hold is asserted at the end (a cryptic position owned by another sample, an own row below the sample's highest level, a
sample without a scaffold, a scaffold of one sample, a scaffold without a site, an N reference position, pulled sites at coverage
0 / 4 / 5, a tie of the pooled counts, a single-base site, two con_bases in both orders, a 5x sample at every site).

usage: python tests/golden/make_pool_golden.py
"""
import os
import sys
import warnings

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                                        # noqa: E402  (the stub importer)

mods = mg.import_reference()
pu, su, lk, fa = mods
import inStrain.polymorpher as pm                               # noqa: E402

NAMES = ["a", "b", "c", "d", "e", "f"]
LENGTHS = [1, 63, 64, 65, 129, 300]
SB = np.r_[0, np.cumsum(LENGTHS)]
SAMPLES = ["s0", "s1", "s2", "s3"]
CH = "ACTG"
rng = np.random.Generator(np.random.PCG64(1401))
ref = rng.integers(0, 4, int(SB[-1]))
seq = np.array(list(CH))[ref]
N_POS = [(5, 10), (5, 11)]                                      # (scaffold, position): reference N
for sc, p in N_POS:
    seq[SB[sc] + p] = "N"
seq = "".join(seq)


def R(sc, p):
    return int(ref[SB[sc] + p])


def alt(sc, p, k=1):
    return (R(sc, p) + k) % 4


# default pile-up of (sample, scaffold): `depth` reads of the reference base at every position ('A' where the reference is N), spread
# over the sample's levels; None = the sample has no read on the scaffold
LEVELS = {"s0": 1, "s1": 2, "s2": 1, "s3": 4}
DEPTH = {"s0": 20, "s1": 16, "s2": 12, "s3": 24}
ABSENT = {("s2", 3)} | {(s, 1) for s in ("s1", "s2", "s3")}     # s2 lacks scaffold d; only s0 has scaffold b
# overrides: (sample, scaffold, position) -> [(mm, base, count), ...] instead of the default column ([] = no read)
O = {}
for s in SAMPLES:                                               # scaffold a (one position): s0 and s1 call it, s2 / s3 pull it
    O[(s, 0, 0)] = [(0, R(0, 0), 10)] + ([(0, alt(0, 0), 10)] if s in ("s0", "s1") else [])
O[("s0", 1, 30)] = [(0, R(1, 30), 10), (0, alt(1, 30), 10)]     # a SNV on the scaffold only s0 has: no site
# scaffold d: a tie of the pooled counts (reference = alternative over the samples): TIE, at the end
# scaffold e
O[("s0", 4, 40)] = [(0, R(4, 40), 12), (0, alt(4, 40), 8), (1, R(4, 40), 200)]     # cryptic in s0 (a SNV at mm 0, none at mm 1) ...
O[("s1", 4, 40)] = [(0, R(4, 40), 10), (1, alt(4, 40), 10)]                         # ... owned by s1
O[("s1", 4, 50)] = [(0, alt(4, 50), 10), (1, R(4, 50), 300)]    # own row at mm 0 (allele_count 1), nothing called at mm 1, not cryptic
O[("s0", 4, 0)] = [(0, alt(4, 0), 11), (0, R(4, 0), 9)]         # bits 0 / 63 / 64 / 128 of the scaffold's words
O[("s3", 4, 63)] = [(0, R(4, 63), 9), (2, alt(4, 63, 2), 9), (3, alt(4, 63, 3), 6)]
O[("s2", 4, 64)] = [(0, alt(4, 64), 12)]
O[("s0", 4, 128)] = [(0, R(4, 128), 10), (0, alt(4, 128), 10)]
O[("s3", 4, 128)] = [(0, R(4, 128), 10), (3, alt(4, 128), 14)]
# scaffold f
O[("s0", 5, 10)] = [(0, 0, 20)]                                 # reference N: every sample with reads there has a row
O[("s1", 5, 10)] = []
O[("s2", 5, 10)] = [(0, 1, 20)]
O[("s3", 5, 10)] = [(0, 0, 3), (1, 0, 1)]                       # (below min_cov: no row, pulled at 4)
O[("s0", 5, 11)] = [(0, 0, 20)]                                 # reference N seen by one sample only: a single-base site
for s in ("s1", "s2", "s3"):
    O[(s, 5, 11)] = []
O[("s0", 5, 100)] = [(0, R(5, 100), 10), (0, alt(5, 100), 10)]  # pulled by the others at coverage 0, 4 and 5
O[("s1", 5, 100)] = []
O[("s2", 5, 100)] = [(0, R(5, 100), 4)]
O[("s3", 5, 100)] = [(0, R(5, 100), 3), (2, R(5, 100), 2)]
O[("s0", 5, 200)] = [(0, alt(5, 200), 14), (0, R(5, 200), 6)]   # con_base alt in s0, reference in s1 ...
O[("s1", 5, 200)] = [(0, R(5, 200), 10), (1, alt(5, 200), 6)]
O[("s0", 5, 201)] = [(0, R(5, 201), 14), (0, alt(5, 201), 6)]   # ... and the other way round
O[("s1", 5, 201)] = [(0, alt(5, 201), 10), (1, R(5, 201), 6)]
O[("s2", 5, 299)] = [(0, alt(5, 299), 12)]                      # the last position; s3 has nothing there
O[("s3", 5, 299)] = []
TIE = (3, 5)
for s, col in (("s0", [(0, R(*TIE), 10), (0, alt(*TIE), 10)]), ("s1", [(0, R(*TIE), 5), (1, alt(*TIE), 5)]), ("s3", [])):
    O[(s, TIE[0], TIE[1])] = col


def observations(sample):
    """-> (pos in the flat space of the six scaffolds, base, mm), one read pair per observation"""
    P, B, M = [], [], []
    for sc in range(len(NAMES)):
        if (sample, sc) in ABSENT:
            continue
        for p in range(LENGTHS[sc]):
            col = O.get((sample, sc, p))
            if col is None:
                base = 0 if seq[SB[sc] + p] == "N" else R(sc, p)
                col = [(k % LEVELS[sample], base, 1) for k in range(DEPTH[sample])]
            for mm, base, n in col:
                P += [SB[sc] + p] * n; B += [base] * n; M += [mm] * n
    return np.array(P, np.int64), np.array(B, np.uint8), np.array(M, np.int64)


class Profile:                                                  # what PoolController reads of an SNVprofile
    def __init__(self, table):
        self.table = table

    def get(self, name):
        assert name == "cumulative_snv_table"
        return self.table.copy()


class SC:                                                       # ... and of a ScaffoldComparison
    def __init__(self, scaffold):
        self.scaffold, self.profiles, self.names = scaffold, [], []


nm = su.generate_snp_model(mg.REF + "/inStrain/helper_files/NullModel.txt", fdr=1e-6)
obs, tables, cols, r2m = {}, {}, {}, {}
for s in SAMPLES:
    pos, base, mm = observations(s)
    obs[s] = (pos, base, mm)
    pair = np.arange(len(pos))
    r2m[s] = {"r%d" % i: int(m) for i, m in zip(pair, mm)}
    parts = []
    for sc, name in enumerate(NAMES):
        k = (pos >= SB[sc]) & (pos < SB[sc + 1])
        if not k.any():
            continue
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _, _, S, _, _ = mg.run_reference_split(mods, name, seq[SB[sc]:SB[sc + 1]], 0, pos[k] - SB[sc], base[k], mm[k], pair[k], nm, min_cov=5)
        cols[(s, name)] = mg.columns_from_obs(pos[k] - SB[sc], base[k], ["r%d" % i for i in pair[k]])
        if len(S):
            parts.append(S)
    tables[s] = pd.concat(parts).reset_index(drop=True)

# the scaffolds that are compared: more than one profile has them (ScaffoldComparison.valid)
scs = []
for sc, name in enumerate(NAMES):
    x = SC(name)
    for s in SAMPLES:
        if (s, name) in cols:
            x.profiles.append(Profile(tables[s])); x.names.append(s)
    if len(x.profiles) > 1:
        scs.append(x)
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    pc = pm.PoolController(scs, {})
    pc.name2scaff2locs, pc.scaff2all_SNVs = pm.extract_SNV_positions(pc.name2snpTable, pc.name2scaffs)
    pulled = {}
    for name, scaff2locs in pc.name2scaff2locs.items():         # pull_SNVS_from_bams on the duck-typed columns
        for scaff, locs in scaff2locs.items():
            got = {c.pos: pm.get_pooling_counts(c, r2m[name]) for c in cols[(name, scaff)] if c.pos in locs}
            for p in set(locs) - set(got):
                got[p] = np.zeros(4, dtype=int)
            pulled.setdefault(scaff, {})[name] = got
    pc.scaff2name2position2counts = pulled
    pc.make_pooled_SNV_table()
    pc.make_pooled_SNV_info_table()
DST, PM = pc.DSTdb, pc.PMdb

# ---- what the inputs hold ----
own = {s: pc.name2snpTable[s] for s in SAMPLES}
raw = {s: tables[s] for s in SAMPLES}


def owns(s, sc, p):
    t = own[s]
    return bool(((t["scaffold"] == NAMES[sc]) & (t["position"] == p)).any())


def dst_row(s, sc, p):
    d = DST[DST["scaffold"] == NAMES[sc]]
    return d.loc[(s, p), ["A", "C", "T", "G"]].to_numpy().astype(int)


t0 = raw["s0"]
assert t0[(t0["scaffold"] == "e") & (t0["position"] == 40)]["cryptic"].all() and not owns("s0", 4, 40) and owns("s1", 4, 40)
r1 = raw["s1"]
low = r1[(r1["scaffold"] == "e") & (r1["position"] == 50)]
assert list(low["mm"]) == [0] and not low["cryptic"].any() and owns("s1", 4, 50)
k = obs["s1"][0] == SB[4] + 50
assert obs["s1"][2][k].max() == 1 and dst_row("s1", 4, 50).sum() == 10 < k.sum()       # own counts, not the all-level counts
assert ("s2", "d") not in cols and "s2" not in set(DST[DST["scaffold"] == "d"].index.get_level_values(0))
assert [s for s in SAMPLES if (s, "b") in cols] == ["s0"] and (t0["scaffold"] == "b").any() and "b" not in set(DST["scaffold"])
assert "c" not in set(DST["scaffold"]) and all((s, "c") in cols for s in SAMPLES)
assert owns("s0", 5, 10) and PM[(PM["scaffold"] == "f") & (PM.index == 10)]["ref_base"].iloc[0] == "N"
assert [int(dst_row(s, 5, 100).sum()) for s in ("s1", "s2", "s3")] == [0, 4, 5] and not any(owns(s, 5, 100) for s in ("s1", "s2", "s3"))
tie = PM[(PM["scaffold"] == "d") & (PM.index == 5)].iloc[0]
top = sorted([tie["A"], tie["C"], tie["T"], tie["G"]])
assert top[-1] == top[-2] > 0
one = PM[(PM["scaffold"] == "f") & (PM.index == 11)].iloc[0]
assert sorted([one["A"], one["C"], one["T"], one["G"]])[:3] == [0, 0, 0] and one["var_base"] == "A" == one["con_base"]
both = set(PM[(PM["scaffold"] == "f") & PM.index.isin([200, 201])]["sample_con_bases"])
a, b = CH[R(5, 200)], CH[alt(5, 200)]
assert len(both) == 2 and all(len(x.split()) == 2 for x in both), both
assert (PM["sample_5x_detections"] >= 1).all()                  # (the reference raises on a site without one)
assert set(DST["scaffold"]) == {"a", "d", "e", "f"} and (PM[PM["scaffold"] == "a"].index == 0).all()

np.savez_compressed(os.path.join(HERE, "pool_obs.npz"), seq=np.array(seq), names=np.array(NAMES), lengths=np.array(LENGTHS),
                    samples=np.array(SAMPLES), **{"%s_%s" % (s, f): v.astype(np.int32) for s in SAMPLES for f, v in zip(("pos", "base", "mm"), obs[s])})
d = DST.copy()
d.index.names = ["sample", "position"]
d.reset_index().to_csv(os.path.join(HERE, "pool_DSTdb.csv"), index=False)
p = PM.copy()
p.index.name = "position"
p.reset_index().to_csv(os.path.join(HERE, "pool_PMdb.csv"), index=False)
print(d.to_string())
print(p.to_string())
print(p.dtypes)
