#!/usr/bin/env python3
"""tests/golden/make_stored_compare_golden.py -- golden vectors of `inStrain compare` on STORED profiles.

Runs ONLY in the build container (needs the reference checkout): imports the reference's own inStrain.readComparer under the stub
importer of make_golden.py and runs its compare_scaffold (readComparer.py:35-143) on inputs in the stored formats -- covT as
SNVprofile._load_special hands it over ({scaffold: {mm: Series}}) and SNP tables as compare_controller.load_cache /
compare_utils.hash_SNP_table do (sorted by scaffold and mm, cut per scaffold).  Three samples over three scaffolds at min_cov 5:

  s0   covT keys {0, 1, 3} on X, {0, 1} on Y, {0, 3} on Z with an EMPTY series under key 3
  s1   covT keys {0, 2}; lacks scaffold Y; one SNV row at mm 1, which is no key of its covT
  s2   covT key {0}; its SNP table is empty

A scaffold is compared among the samples whose covT names it (ScaffoldComparison.add_profile over _get_covt_keys).  Only data is
stored: the inputs (stored_compare_inputs.npz) and the reference's two tables (stored_compare_table.csv, stored_compare_mdb.csv).

usage: python tests/golden/make_stored_compare_golden.py
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
import inStrain.compare_utils as cu                             # noqa: E402
import inStrain.readComparer as rc                              # noqa: E402

NAMES = ["X", "Y", "Z"]
LENGTHS = [130, 64, 200]
SAMPLES = ["s0", "s1", "s2"]
KEYS = {("s0", "X"): [0, 1, 3], ("s0", "Y"): [0, 1], ("s0", "Z"): [0, 3],
        ("s1", "X"): [0, 2], ("s1", "Z"): [0, 2],
        ("s2", "X"): [0], ("s2", "Y"): [0], ("s2", "Z"): [0]}
EMPTY = {("s0", "Z", 3)}
CH = "ACTG"
rng = np.random.Generator(np.random.PCG64(1601))

# ---- covT: sparse series of small coverages, so that min_cov 5 is reached at some positions only by cumulation ----
covT = {s: {} for s in SAMPLES}
for (s, n), mms in KEYS.items():
    length = LENGTHS[NAMES.index(n)]
    d = {}
    for mm in mms:
        if (s, n, mm) in EMPTY:
            d[mm] = pd.Series(np.zeros(0, dtype="int32"), index=np.zeros(0, dtype="int"))
            continue
        p = np.flatnonzero(rng.random(length) < (0.9 if mm == 0 else 0.5))
        p = np.union1d(p, [0, length - 1]) if mm == 0 else p    # the first and the last position are covered
        d[mm] = pd.Series(rng.integers(1, 9, size=len(p)).astype("int32"), index=p.astype("int"))
    covT[s][n] = d


# ---- SNP tables ----
def snv_rows(s, n, positions, mms):
    rows = []
    for p in positions:
        ref = int(rng.integers(0, 4))
        for mm in sorted(rng.choice(mms, size=int(rng.integers(1, len(mms) + 1)), replace=False).tolist()):
            cnt = rng.integers(0, 7, size=4)
            con = int(rng.integers(0, 4))
            cnt[con] += int(rng.integers(6, 30))
            var = int((con + rng.integers(1, 4)) % 4)
            two = bool(rng.random() < 0.6)
            if two:
                cnt[var] += int(rng.integers(2, 12))
            rows.append({"scaffold": n, "position": int(p), "position_coverage": int(cnt.sum()), "allele_count": 2 if two else 1,
                         "ref_base": CH[ref], "con_base": CH[con], "var_base": CH[var], "A": int(cnt[0]), "C": int(cnt[1]),
                         "T": int(cnt[2]), "G": int(cnt[3]), "mm": int(mm)})
    return rows


shared = {n: rng.choice(LENGTHS[NAMES.index(n)], size=14, replace=False) for n in NAMES}   # positions both s0 and s1 may call
tables = {}
r0, r1 = [], []
for n in NAMES:
    own0 = np.union1d(shared[n][:10], [0, LENGTHS[NAMES.index(n)] - 1])
    r0 += snv_rows("s0", n, own0, KEYS[("s0", n)])
    if ("s1", n) in KEYS:
        r1 += snv_rows("s1", n, shared[n][5:], [0, 2])
r1.append(dict(r1[0], mm=1))                                    # a row whose mm is no key of s1's covT: the highest-mm row of ITS position
r1[-1]["position"] = int(shared["X"][12])                       # ... where s1 also has lower rows
r1 = [r for r in r1 if not (r["scaffold"] == "X" and r["position"] == int(shared["X"][12]) and r["mm"] > 1)]
tables["s0"] = pd.DataFrame(r0).sample(frac=1, random_state=3).reset_index(drop=True)      # stored order is not sorted by mm
tables["s1"] = pd.DataFrame(r1).sample(frac=1, random_state=4).reset_index(drop=True)
tables["s2"] = pd.DataFrame()

nm = su.generate_snp_model(mg.REF + "/inStrain/helper_files/NullModel.txt", fdr=1e-6)
hashed = {s: cu.hash_SNP_table(tables[s]) for s in SAMPLES}
cdbs, mdbs = [], []
for n, length in zip(NAMES, LENGTHS):
    cur = [s for s in SAMPLES if n in covT[s]]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        (Cdb, Mdb, _, name), _ = rc.compare_scaffold(n, cur, [hashed[s].get(n, pd.DataFrame()) for s in cur], [covT[s][n] for s in cur],
                                                      length, nm, min_cov=5, min_freq=0.05, store_mismatch_locations=True)
    assert name == n
    cdbs.append(Cdb)
    mdbs.append(Mdb)
Cdb = pd.concat(cdbs).reset_index(drop=True)
Mdb = pd.concat(mdbs).reset_index(drop=True)
Mdb = Mdb[["scaffold", "name1", "name2", "mm", "position", "consensus_SNP", "population_SNP"]]
Mdb = Mdb.astype({"position": "int64", "mm": "int64"}).sort_values(["name1", "name2", "scaffold", "mm", "position"]).reset_index(drop=True)

# ---- what the inputs hold ----
x1 = tables["s1"][(tables["s1"]["scaffold"] == "X") & (tables["s1"]["position"] == int(shared["X"][12]))]
assert x1["mm"].max() == 1 and 1 not in covT["s1"]["X"] and len(x1) >= 1
assert len(covT["s0"]["Z"][3]) == 0 and 3 in set(Cdb[(Cdb["scaffold"] == "Z")]["mm"])
assert set(Cdb[Cdb["scaffold"] == "Y"]["name1"]) == {"s0"} and set(Cdb[Cdb["scaffold"] == "Y"]["name2"]) == {"s2"}
assert sorted(set(Cdb[(Cdb["scaffold"] == "X") & (Cdb["name1"] == "s0") & (Cdb["name2"] == "s1")]["mm"])) == [0, 1, 2, 3]
assert (Cdb["consensus_SNPs"] > 0).any() and (Cdb["population_SNPs"] > 0).any() and (Cdb["consensus_SNPs"] != Cdb["population_SNPs"]).any()
assert len(Mdb) > 0 and {("s0", "s1"), ("s0", "s2"), ("s1", "s2")} == set(zip(Mdb["name1"], Mdb["name2"]))
cum = covT["s0"]["X"][0].add(covT["s0"]["X"][1], fill_value=0)
assert ((cum >= 5) & ~(covT["s0"]["X"][0].reindex(cum.index, fill_value=0) >= 5)).any()        # covered only by cumulation

arrays = {"names": np.array(NAMES), "lengths": np.array(LENGTHS), "samples": np.array(SAMPLES)}
for s in SAMPLES:
    sc, mmv, off, pos, val = [], [], [0], [], []
    for n in NAMES:
        for mm, ser in covT[s].get(n, {}).items():
            sc.append(NAMES.index(n)); mmv.append(mm)
            pos.append(ser.index.to_numpy()); val.append(ser.to_numpy())
            off.append(off[-1] + len(ser))
    arrays.update({s + "_cov_scaffold": np.array(sc, np.int32), s + "_cov_mm": np.array(mmv, np.int32), s + "_cov_off": np.array(off, np.int64),
                   s + "_cov_pos": np.concatenate(pos).astype(np.int32), s + "_cov_val": np.concatenate(val).astype(np.int32)})
    t = tables[s]
    if len(t):
        arrays.update({s + "_snv_" + c: t[c].to_numpy() if t[c].dtype != object else t[c].to_numpy().astype(str) for c in t.columns})
np.savez_compressed(os.path.join(HERE, "stored_compare_inputs.npz"), **arrays)
Cdb.to_csv(os.path.join(HERE, "stored_compare_table.csv"), index=False)
Mdb.to_csv(os.path.join(HERE, "stored_compare_mdb.csv"), index=False)
print(Cdb.to_string())
print(Mdb.to_string())
