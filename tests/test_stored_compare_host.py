"""CPU: the host side of comparing stored profiles -- compare.pack_profile (numpy only), the golden fixture of
tests/golden/make_stored_compare_golden.py against oracle/compare.py, and the store_sample / load_sample round trip."""
import itertools
import os

import numpy as np
import pandas as pd
import pytest

from instrain_amd import _lib, compare
from instrain_amd.profile import emitters
from tests import stored_ref, util

INDEX = {"a": 0, "b": 1, "c": 2}
LENGTHS = [100, 64, 300]


def _ser(pos, val):
    return pd.Series(np.asarray(val, dtype="int32"), index=np.asarray(pos, dtype="int"))


def _snv(**over):
    row = {"scaffold": "a", "position": 5, "position_coverage": 12, "allele_count": 2, "ref_base": "A", "con_base": "C", "var_base": "A",
           "A": 4, "C": 8, "T": 0, "G": 0, "mm": 1}
    row.update(over)
    return row


COVT = {"c": {0: _ser([1, 2, 299], [3, 4, 5]), 2: _ser([2], [9])},
        "a": {1: _ser([0, 99], [1, 2]), 0: _ser([7], [6])},
        "nowhere": {5: _ser([0], [1])},
        "b": {}}


def test_levels_are_the_union_and_the_series_follow_in_csr_order():
    p = compare.pack_profile(INDEX, LENGTHS, COVT, None)
    assert p["scaffolds"] == ["a", "c"] and p["ids"].tolist() == [0, 2]          # set order; `nowhere` and the key-less `b` are left out
    assert p["levels"].tolist() == [0, 1, 2] and p["levels"].dtype == np.int32    # (5 is a key of a scaffold the set does not name)
    assert p["present"].tolist() == [[1, 1, 0], [1, 0, 1]]
    assert p["offsets"].tolist() == [0, 1, 3, 3, 6, 6, 7]
    assert p["positions"].tolist() == [7, 0, 99, 1, 2, 299, 2] and p["values"].tolist() == [6, 1, 2, 3, 4, 5, 9]
    assert p["positions"].dtype == p["values"].dtype == np.uint32 and p["offsets"].dtype == np.int64 and len(p["snv"]) == 0
    q = compare.pack_profile(INDEX, LENGTHS, COVT, pd.DataFrame(), mm_values=[0, 1, 2, 7])
    assert q["levels"].tolist() == [0, 1, 2, 7] and q["present"].tolist() == [[1, 1, 0, 0], [1, 0, 1, 0]]
    assert q["offsets"].tolist() == [0, 1, 3, 3, 3, 6, 6, 7, 7] and q["positions"].tolist() == p["positions"].tolist()
    with pytest.raises(ValueError):                              # a key mm_values does not name
        compare.pack_profile(INDEX, LENGTHS, COVT, None, mm_values=[0, 1])
    with pytest.raises(ValueError):
        compare.pack_profile(INDEX, LENGTHS, COVT, None, mm_values=[0, 2, 1])
    empty = compare.pack_profile(INDEX, LENGTHS, {}, None)
    assert empty["scaffolds"] == [] and len(empty["levels"]) == 0 and empty["offsets"].tolist() == [0]
    assert compare.pack_profile(INDEX, LENGTHS, None, None)["scaffolds"] == []


def test_tuples_and_an_unsorted_series():
    covT = {"a": {0: (np.array([9, 3, 50]), np.array([1, 2, 3])), 4: _ser([], [])}}
    p = compare.pack_profile(INDEX, LENGTHS, covT, None)
    assert p["positions"].tolist() == [3, 9, 50] and p["values"].tolist() == [2, 1, 3]
    assert p["levels"].tolist() == [0, 4] and p["present"].tolist() == [[1, 1]] and p["offsets"].tolist() == [0, 3, 3]    # an empty series keeps its key
    big = compare.pack_profile(INDEX, LENGTHS, {"a": {0: (np.array([1]), np.array([2 ** 32 - 1], dtype=np.uint64))}}, None)
    assert big["values"].tolist() == [2 ** 32 - 1]


@pytest.mark.parametrize("series", [
    (np.array([3, 3]), np.array([1, 1])),                       # a position twice
    (np.array([5, 3, 5]), np.array([1, 1, 1])),                 # ... in an unsorted series
    (np.array([3, 4]), np.array([1, -1])),                      # a negative value
    (np.array([-1, 4]), np.array([1, 1])),                      # a negative position
    (np.array([3, 4]), np.array([1.0, np.nan])),                # NaN
    (np.array([3, 4]), np.array([1.0, 2.5])),                   # no whole number
    (np.array([3.5, 4]), np.array([1, 2])),
    (np.array([3, 100]), np.array([1, 2])),                     # beyond the set's length of the scaffold
    (np.array([3, 4]), np.array([1, 2 ** 32])),                 # more than a counter holds
    (np.array([3, 4]), np.array([1])),                          # not one value per position
])
def test_bad_series_are_refused(series):
    with pytest.raises(ValueError):
        compare.pack_profile(INDEX, LENGTHS, {"a": {0: series}}, None)


def test_snv_rows():
    covT = {"a": {0: _ser([5], [9])}, "c": {0: _ser([0], [9])}}
    db = pd.DataFrame([_snv(), _snv(scaffold="c", position=299, ref_base="N", con_base="G", var_base="T", A=0, C=0, T=1, G=11, mm=0, allele_count=1),
                       _snv(scaffold="b"), _snv(scaffold="nowhere"), _snv(position=6, mm=65535)])
    p = compare.pack_profile(INDEX, LENGTHS, covT, db)
    s = p["snv"]
    assert s.dtype == _lib.PROFILE_SNV_DT and len(s) == 3          # `b` has no covT entry in this sample, `nowhere` is not in the set
    assert s["scaffold"].tolist() == [0, 1, 0] and s["position"].tolist() == [5, 299, 6] and s["mm"].tolist() == [1, 0, 65535]
    assert s["con_base"].tolist() == [1, 3, 1] and s["ref_base"].tolist() == [0, 4, 0] and s["var_base"].tolist() == [0, 2, 0]
    assert s["allele_count"].tolist() == [2, 1, 2] and s["cnt"].tolist() == [[4, 8, 0, 0], [0, 0, 1, 11], [4, 8, 0, 0]]
    # the old column names, as the reference renames them; categorical columns as profile_bam's tables have them
    old = db.rename(columns={"con_base": "conBase", "ref_base": "refBase", "var_base": "varBase", "position_coverage": "baseCoverage"})
    old = old.astype({"scaffold": "category", "conBase": "category"})
    assert compare.pack_profile(INDEX, LENGTHS, covT, old)["snv"].tobytes() == s.tobytes()
    assert compare.pack_profile(INDEX, LENGTHS, covT, db.drop(columns=["position_coverage"]))["snv"].tobytes() == s.tobytes()
    for bad in (_snv(position_coverage=13), _snv(con_base="N"), _snv(var_base="X"), _snv(ref_base="n"), _snv(position=100), _snv(position=-1),
                _snv(mm=65536), _snv(mm=-1), _snv(A=-4, position_coverage=4), _snv(A=np.nan), _snv(allele_count=300)):
        with pytest.raises(ValueError):
            compare.pack_profile(INDEX, LENGTHS, covT, pd.DataFrame([_snv(), bad]))
    with pytest.raises(ValueError):
        compare.pack_profile(INDEX, LENGTHS, covT, db.drop(columns=["G"]))
    assert len(compare.pack_profile(INDEX, LENGTHS, covT, pd.DataFrame([_snv(scaffold="b")]))["snv"]) == 0


# ---- the golden fixture is neither vacuous nor wrong: oracle/compare.py reproduces the reference's tables from its inputs ----
ORACLE_SNV_DT = np.dtype([("pos", "<i8"), ("mm", "<i8"), ("con_base", "<i8"), ("ref_base", "<i8"), ("var_base", "<i8"), ("allele_count", "<i8"),
                          ("position_coverage", "<i8"), ("cnt", "<i8", (4,))])
ORACLE_ENTRY_DT = np.dtype([("pos", "<i8"), ("mm", "<i8"), ("cnt", "<i8", (4,))])
CODE = {"A": 0, "C": 1, "T": 2, "G": 3, "N": 4}


def _oracle_inputs(covT_sc, table, scaffold):
    e = np.zeros(sum(len(s) for s in covT_sc.values()), dtype=ORACLE_ENTRY_DT)
    at = 0
    for mm, ser in covT_sc.items():
        e["pos"][at:at + len(ser)], e["mm"][at:at + len(ser)], e["cnt"][at:at + len(ser), 0] = ser.index.to_numpy(), mm, ser.to_numpy()
        at += len(ser)
    t = table[table["scaffold"] == scaffold] if len(table) else table
    s = np.zeros(len(t), dtype=ORACLE_SNV_DT)
    if len(t):
        s["pos"], s["mm"], s["allele_count"], s["position_coverage"] = t["position"], t["mm"], t["allele_count"], t["position_coverage"]
        for c in ("con_base", "ref_base", "var_base"):
            s[c] = [CODE[b] for b in t[c]]
        for j, b in enumerate("ACTG"):
            s["cnt"][:, j] = t[b]
    return e, s


def test_the_golden_tables_follow_from_the_golden_inputs_by_the_oracle():
    from oracle import compare as ocompare
    lut, fb = util.load_lut()
    names, lengths, samples, covT, tables = stored_ref.load_stored_golden(os.path.join(util.GOLD, "stored_compare_inputs.npz"))
    gold_t = pd.read_csv(os.path.join(util.GOLD, "stored_compare_table.csv"), float_precision="round_trip")
    gold_m = pd.read_csv(os.path.join(util.GOLD, "stored_compare_mdb.csv"))
    exp_t, exp_m = [], []
    for n, length in zip(names, lengths):
        for a, b in itertools.combinations([s for s in samples if n in covT[s]], 2):
            ea, sa = _oracle_inputs(covT[a][n], tables[a], n)
            eb, sb = _oracle_inputs(covT[b][n], tables[b], n)
            o, c = ocompare.calc_mm2overlap(ea, eb, length, min_cov=5)
            for mm in sorted(set(covT[a][n]) | set(covT[b][n])):    # a key with an empty series has no entry the oracle could see: carried
                if mm not in o:
                    below = max(k for k in o if k < mm)
                    o[mm], c[mm] = o[below], c[below]
            rows = ocompare.compare_snp_tables(sa, sb, o, lut, fb, min_freq=0.05)
            exp_m += [(n, a, b, mm, p, cc, q) for mm, p, cc, q in rows]
            exp_t += [(n, a, b, t["mm"], t["compared_bases_count"], t["consensus_SNPs"], t["population_SNPs"], t["coverage_overlap"],
                       t["percent_genome_compared"], t["length"]) for t in ocompare.overlap_table(o, c, rows, length)]
    g = gold_t.sort_values(["scaffold", "name1", "name2", "mm"])
    got_t = list(zip(g["scaffold"], g["name1"], g["name2"], g["mm"], g["compared_bases_count"], g["consensus_SNPs"], g["population_SNPs"],
                     g["coverage_overlap"], g["percent_genome_compared"], g["length"]))
    assert len(got_t) == len(exp_t) == 18
    for x, y in zip(got_t, sorted(exp_t)):
        assert x == y
    got_m = sorted(zip(gold_m["scaffold"], gold_m["name1"], gold_m["name2"], gold_m["mm"], gold_m["position"],
                       gold_m["consensus_SNP"].astype(bool), gold_m["population_SNP"].astype(bool)))
    assert got_m == sorted(exp_m) and len(got_m) > 20
    # what the issue asks the inputs to hold
    assert [sorted(covT[s]["X"]) for s in samples] == [[0, 1, 3], [0, 2], [0]] and len(covT["s0"]["Z"][3]) == 0 and "Y" not in covT["s1"]
    assert len(tables["s2"]) == 0 and 1 in set(tables["s1"]["mm"]) and 1 not in covT["s1"]["X"]


def _have_hdf5():
    try:
        emitters._backend()
        return True
    except Exception:
        return False


class _Profile:
    def __init__(self, scaffold, covT, table):
        self.scaffold, self.covT, self.cumulative_snv_table, self.cumulative_scaffold_table = scaffold, covT, table, None


@pytest.mark.skipif(not _have_hdf5(), reason="no h5py / libhdf5 on this host")
def test_store_and_load_a_sample(tmp_path):
    names, lengths, samples, covT, tables = stored_ref.load_stored_golden(os.path.join(util.GOLD, "stored_compare_inputs.npz"))
    index = {n: i for i, n in enumerate(names)}
    for s in samples:
        t = tables[s]
        profs = [_Profile(n, covT[s][n], t[t["scaffold"] == n] if len(t) else pd.DataFrame()) for n in names if n in covT[s]]
        folder = str(tmp_path / s / "raw_data")
        paths = compare.store_sample(folder, profs)
        assert [os.path.basename(p) for p in paths] == ["covT.hd5", "cumulative_snv_table.csv.gz"]
        got_c, got_t = compare.load_sample(folder)
        a, b = compare.pack_profile(index, lengths, covT[s], t), compare.pack_profile(index, lengths, got_c, got_t)
        assert a["scaffolds"] == b["scaffolds"]
        for k in ("ids", "levels", "present", "offsets", "positions", "values"):
            assert a[k].tobytes() == b[k].tobytes(), (s, k)
        order = lambda r: r[np.lexsort((r["mm"], r["position"], r["scaffold"]))]
        assert order(a["snv"]).tobytes() == order(b["snv"]).tobytes()
        only_c, only_t = compare.load_sample(folder, scaffolds=["Z"])
        assert set(only_c) == {"Z"} and (len(only_t) == 0 or set(only_t["scaffold"]) == {"Z"})
