"""CPU-only: a stored profile's host side (instrain_amd/profile/stored.py) -- pack_levels against arrays written out by hand, every
ValueError it promises, the store_profile / load_profile round trip, the chunking and table layouts, and isx_stored_create without a GPU."""
import ctypes as C
import types

import numpy as np
import pandas as pd
import pytest

from instrain_amd import _lib, compare
from instrain_amd.profile import emitters, stored


def _have_hdf5():
    try:
        emitters._backend()
        return True
    except RuntimeError:
        return False


def _ser(values, index, dtype):
    return pd.Series(np.asarray(values, dtype=dtype), index=np.asarray(index, dtype=np.int64))


def _profile():
    """a (10), b (6), c (4): a's covT index is unsorted and its key 2 has an empty series; b exists at the top level only and comes as
    tuples; no table names c; clonT's keys are a strict subset of covT's on a"""
    covT = {"a": {0: _ser([3, 1, 2], [5, 0, 9], "int32"), 2: _ser([], [], "int32")},
            "b": {5: (np.array([1, 4]), np.array([7, 8]))}}
    clonT = {"a": {0: _ser([1.0, 0.5], [0, 5], "float32")}, "b": {5: (np.array([4]), np.array([0.25], dtype=np.float32))}}
    clonTR = {"a": {0: _ser([0.75], [5], "float32")}}
    return covT, clonT, clonTR


def test_pack_levels_equals_arrays_written_by_hand():
    covT, clonT, clonTR = _profile()
    p = stored.pack_levels(["a", "b", "c"], [10, 6, 4], covT, clonT, clonTR)
    assert p["scaffolds"] == ["a", "b", "c"]
    exp = {"bounds": np.array([0, 10, 16, 20], np.int64), "levels": np.array([0, 2, 5], np.int32),
           "cov_present": np.array([[1, 1, 0], [0, 0, 1], [0, 0, 0]], np.uint8),
           "clon_present": np.array([[1, 0, 0], [0, 0, 1], [0, 0, 0]], np.uint8),
           "cov_offsets": np.array([0, 3, 3, 5], np.int64), "cov_gpos": np.array([0, 5, 9, 11, 14], np.uint32),
           "cov_values": np.array([1, 3, 2, 7, 8], np.uint32),
           "clon_offsets": np.array([0, 2, 2, 3], np.int64), "clon_gpos": np.array([0, 5, 14], np.uint32),
           "clon_values": np.array([1.0, 0.5, 0.25], np.float32),
           "clonr_offsets": np.array([0, 1, 1, 1], np.int64), "clonr_gpos": np.array([5], np.uint32),
           "clonr_values": np.array([0.75], np.float32)}
    assert set(p) == set(exp) | {"scaffolds"}
    for k, e in exp.items():
        assert p[k].dtype == e.dtype and np.array_equal(p[k], e), k
    # the order given is the order of the flat space; mm_values may name more levels than the tables have
    q = stored.pack_levels(["c", "b"], [4, 6], covT, clonT, clonTR, mm_values=[0, 5, 9])
    assert np.array_equal(q["bounds"], [0, 4, 10]) and np.array_equal(q["levels"], [0, 5, 9])
    assert np.array_equal(q["cov_present"], [[0, 0, 0], [0, 1, 0]]) and np.array_equal(q["cov_offsets"], [0, 0, 2, 2])
    assert np.array_equal(q["cov_gpos"], [5, 8]) and np.array_equal(q["clon_gpos"], [8]) and len(q["clonr_gpos"]) == 0
    # without clonT / clonTR the two CSRs are empty, level by level
    r = stored.pack_levels(["a"], [10], covT)
    assert np.array_equal(r["clon_offsets"], [0, 0, 0]) and np.array_equal(r["clonr_offsets"], [0, 0, 0]) and not r["clon_present"].any()


@pytest.mark.parametrize("table,series,needle", [
    ("covT", _ser([1, 2], [3, 3], "int32"), "twice"),
    ("covT", _ser([1], [10], "int32"), "positions"),
    ("covT", _ser([1.5], [1], "float64"), "values"),
    ("covT", _ser([-1], [1], "int64"), "values"),
    ("covT", _ser([np.nan], [1], "float64"), "values"),
    ("clonT", _ser([np.nan], [1], "float32"), "clonality"),
    ("clonT", _ser([0.0], [1], "float32"), "clonality"),
    ("clonT", _ser([1.5], [1], "float32"), "clonality"),
    ("clonT", _ser([0.5, 0.5], [2, 2], "float32"), "twice"),
    ("clonTR", _ser([0.5], [10], "float32"), "positions"),
    ("clonTR", _ser([-0.5], [1], "float32"), "clonality"),
])
def test_pack_levels_refuses_and_names_the_series(table, series, needle):
    tables = {"covT": {"a": {0: _ser([1], [0], "int32")}}, "clonT": None, "clonTR": None}
    tables[table] = {"a": {1: series}}
    with pytest.raises(ValueError) as e:
        stored.pack_levels(["a"], [10], tables["covT"], tables["clonT"], tables["clonTR"])
    assert "%s['a'][1]" % table in str(e.value) and needle in str(e.value), str(e.value)


def test_pack_levels_refuses_keys_outside_mm_values_and_bad_axes():
    covT, clonT, clonTR = _profile()
    with pytest.raises(ValueError, match=r"\[5\]"):
        stored.pack_levels(["a", "b"], [10, 6], covT, clonT, clonTR, mm_values=[0, 2])
    with pytest.raises(ValueError, match="ascend"):
        stored.pack_levels(["a"], [10], covT, mm_values=[2, 0])
    with pytest.raises(ValueError, match="length"):
        stored.pack_levels(["a", "b"], [10], covT)
    with pytest.raises(ValueError, match="2\\^32"):
        stored.pack_levels(["a", "b"], [1 << 31, 1 << 31], {})


def test_chunks_and_level_ranks():
    assert stored.chunk_scaffolds("abcde", [5, 5, 11, 3, 3], 10) == [[0, 1], [2], [3, 4]]
    assert stored.chunk_scaffolds("ab", [5, 5], 1 << 20) == [[0, 1]] and stored.chunk_scaffolds([], [], 10) == []
    covT, clonT, clonTR = _profile()
    assert stored.profile_levels({"covT": covT, "clonT": clonT, "clonTR": clonTR}) == [0, 2, 5]
    assert stored.profile_levels({}) == [0]
    sdb = pd.DataFrame({"scaffold": ["b", "a", "a", "zz"], "position": [2, 7, 7, 0], "mm": [5, 2, 0, 0], "allele_count": [2, 1, 2, 1],
                        "class": ["SNV", "SNS", "con_SNV", "SNS"], "con_base": list("ACGT"), "var_base": list("CCAA"),
                        "ref_base": list("AANT"), "A": [1, 2, 3, 4], "C": [0, 0, 0, 0], "T": [0, 0, 0, 0], "G": [9, 8, 7, 6], "cryptic": False})
    v = stored.snv_rows(sdb, {"a": 0, "b": 10}, [0, 2, 5])
    from instrain_amd.profile.snv_utilities import CLASSES
    assert v["gpos"].tolist() == [7, 7, 12] and v["mm"].tolist() == [0, 1, 2] and v["allele_count"].tolist() == [2, 1, 2]
    assert v["cls"].tolist() == [CLASSES.index("con_SNV"), CLASSES.index("SNS"), CLASSES.index("SNV")]
    assert v["ref_base"].tolist() == [4, 0, 0] and v["cnt"][:, 3].tolist() == [7, 8, 9]
    with pytest.raises(ValueError, match="no level"):
        stored.snv_rows(sdb, {"a": 0, "b": 10}, [0, 5])
    ldb = pd.DataFrame({"scaffold": ["b", "a"], "position_A": [1, 2], "position_B": [4, 3], "mm": [5, 0], "r2": [0.5, np.nan],
                        "d_prime": [1.0, 0.25], "total": [20, 30]})
    l = stored.ld_rows(ldb, {"a": 0, "b": 10}, [0, 2, 5])
    assert l["gpos_a"].tolist() == [2, 11] and l["gpos_b"].tolist() == [3, 14] and l["mm"].tolist() == [0, 2]
    assert np.isnan(l["r2"][0]) and l["d_prime"].tolist() == [0.25, 1.0] and np.isnan(l["r2_normalized"]).all()
    assert len(stored.snv_rows(pd.DataFrame(), {"a": 0}, [0])) == 0 and len(stored.ld_rows(None, {"a": 0}, [0])) == 0


@pytest.mark.skipif(not _have_hdf5(), reason="no h5py / libhdf5 on this host")
def test_store_profile_load_profile_round_trip(tmp_path):
    covT, clonT, clonTR = _profile()
    covT["b"] = {5: _ser([7, 8], [1, 4], "int32")}
    clonT["b"] = {5: _ser([0.25], [4], "float32")}
    covT["a"][0] = covT["a"][0].sort_index()
    snv = pd.DataFrame({"scaffold": ["a", "a"], "position": [5, 9], "mm": [0, 2], "con_base": ["A", "C"], "ref_base": ["A", "A"],
                        "var_base": ["C", "A"], "allele_count": [2, 1], "A": [2, 0], "C": [1, 2], "T": [0, 0], "G": [0, 0],
                        "position_coverage": [3, 2], "class": ["SNV", "SNS"], "cryptic": [False, False], "var_freq": [1 / 3, 0.0]})
    ld = pd.DataFrame({"scaffold": ["a"], "position_A": [5], "position_B": [9], "mm": [2], "r2": [0.1 + 0.2], "d_prime": [np.nan], "distance": [4]})
    st_a = pd.DataFrame({"scaffold": ["a", "a"], "length": [10, 10], "coverage": [0.6, 0.6], "mm": [0, 2]})
    st_b = pd.DataFrame({"scaffold": ["b"], "length": [6], "coverage": [2.5], "mm": [5]})
    profs = [types.SimpleNamespace(scaffold="a", covT=covT["a"], clonT=clonT["a"], clonTR=clonTR["a"], cumulative_snv_table=snv,
                                   raw_linkage_table=ld, cumulative_scaffold_table=st_a),
             types.SimpleNamespace(scaffold="b", covT=covT["b"], clonT=clonT["b"], clonTR={}, cumulative_snv_table=pd.DataFrame(),
                                   raw_linkage_table=pd.DataFrame(), cumulative_scaffold_table=st_b)]
    folder = str(tmp_path / "raw_data")
    paths = stored.store_profile(folder, profs, scaffold2length={"a": 10, "b": 6, "c": 4})
    assert sorted(p.rsplit("/", 1)[1] for p in paths.values()) == sorted(
        ["covT.hd5", "clonT.hd5", "clonTR.hd5", "cumulative_snv_table.csv.gz", "raw_linkage_table.csv.gz",
         "cumulative_scaffold_table.csv.gz", "scaffold2length.json"])
    got = stored.load_profile(folder)
    for name, exp in (("covT", covT), ("clonT", clonT), ("clonTR", clonTR)):
        assert {s: sorted(d) for s, d in got[name].items()} == {s: sorted(d) for s, d in exp.items()}, name
        for s, d in exp.items():
            for mm, ser in d.items():
                pd.testing.assert_series_equal(got[name][s][mm], ser, check_exact=True, check_index_type=False)
    pd.testing.assert_frame_equal(got["cumulative_snv_table"], snv, check_exact=True)
    pd.testing.assert_frame_equal(got["raw_linkage_table"], ld, check_exact=True)
    pd.testing.assert_frame_equal(got["cumulative_scaffold_table"], pd.concat([st_a, st_b]).reset_index(drop=True), check_exact=True)
    assert got["scaffold2length"] == {"a": 10, "b": 6, "c": 4} and list(got["scaffold2length"]) == ["a", "b", "c"]
    only_b = stored.load_profile(folder, scaffolds=["b"])
    assert list(only_b["covT"]) == ["b"] and len(only_b["cumulative_snv_table"]) == 0 and only_b["scaffold2length"] == {"b": 6}
    # what comes back packs to what the originals pack to
    a, b = (stored.pack_levels(["a", "b", "c"], [10, 6, 4], x["covT"], x["clonT"], x["clonTR"])
            for x in (got, {"covT": covT, "clonT": clonT, "clonTR": clonTR}))
    for k in b:
        assert np.array_equal(a[k], b[k]), k
    # compare.load_sample still reads the folder
    c2, s2 = compare.load_sample(folder)
    assert sorted(c2) == ["a", "b"] and np.array_equal(c2["a"][0].to_numpy(), covT["a"][0].to_numpy()) and len(s2) == 2
    # a folder with nothing in it: empty tables, no error
    empty = stored.load_profile(str(tmp_path / "nothing"))
    assert empty["covT"] == {} and len(empty["raw_linkage_table"]) == 0 and "scaffold2length" not in empty


def test_stored_create_without_a_gpu_is_a_loud_error_not_a_fallback():
    """no MI355X, no context: isx_stored_create says so and hands nothing back (there is no CPU path in the product)"""
    import torch
    if torch.cuda.is_available():
        return
    lib = _lib.load()
    ctx = C.c_void_p()
    assert lib.isx_ctx_create(0, C.byref(ctx)) != 0 and not ctx.value
    covT, clonT, clonTR = _profile()
    p = stored.pack_levels(["a", "b", "c"], [10, 6, 4], covT, clonT, clonTR)
    h = C.c_void_p(1)
    rc = lib.isx_stored_create(None, 3, p["bounds"].ctypes.data, 3, p["cov_present"].ctypes.data, p["clon_present"].ctypes.data,
                               p["cov_offsets"].ctypes.data, p["cov_gpos"].ctypes.data, p["cov_values"].ctypes.data,
                               p["clon_offsets"].ctypes.data, p["clon_gpos"].ctypes.data, p["clon_values"].ctypes.data,
                               p["clonr_offsets"].ctypes.data, p["clonr_gpos"].ctypes.data, p["clonr_values"].ctypes.data, None, C.byref(h))
    assert rc != 0 and not h.value
    msg = lib.isx_last_error().lower()
    assert b"isx_stored_create" in msg and (b"device" in msg or b"ctx" in msg)
