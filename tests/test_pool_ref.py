"""CPU-only: SNV pooling across samples (`compare --bams`).  tests/pool_ref.py -- the restatement the GPU tests compare the device with --
against the reference's own DSTdb / PMdb (tests/golden/make_pool_golden.py), the two user tables (compare.pooled_SNV_info /
pooled_SNV_data) on those frames, and profile_bam's hook that hands every collected batch to SampleSet.pool_add before its release."""
import os
import types

import numpy as np
import pandas as pd
import pytest

from instrain_amd import _lib, compare
from instrain_amd.profile import profile_utilities as pu
from tests import pool_ref, util
from tests.test_profile_driver_host import World

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "pool_obs.npz"))
    names, lengths, samples = [str(n) for n in g["names"]], g["lengths"].tolist(), [str(s) for s in g["samples"]]
    dst, pm = pool_ref.load_golden(GOLDEN, names)
    return dict(names=names, lengths=lengths, seq=str(g["seq"]), dst=dst, pm=pm,
                samples=[(s, g[s + "_pos"], g[s + "_base"], g[s + "_mm"]) for s in samples])


def test_restatement_equals_the_reference(golden):
    lut, fb = util.load_lut()
    dst, pm = pool_ref.pooled_tables(golden["samples"], golden["seq"], golden["names"], golden["lengths"], lut, fb)
    pool_ref.same_frames(dst, golden["dst"])
    pool_ref.same_frames(pm, golden["pm"])
    # what the golden inputs were chosen for is really in the tables
    assert list(pm["scaffold"].cat.categories) == ["a", "d", "e", "f"] and len(pm) == 14 and len(dst) == 4 + 3 + 24 + 24
    assert set(pm["sample_con_bases"]) >= {"['G' 'T']", "['G' 'A']", "['A']"} and (pm["sample_5x_detections"] >= 1).all()
    assert "N" in set(pm["ref_base"]) and ((pm["con_base"] == "A") & (pm["var_base"] == "A")).any()
    assert sorted(dst.xs(100, level=1)[["A", "C", "T", "G"]].sum(axis=1).tolist()) == [0, 4, 5, 20]


def test_pooled_SNV_info(golden):
    info = compare.pooled_SNV_info(golden["pm"])
    assert list(info.columns) == ["scaffold", "position", "depth", "A", "C", "T", "G", "ref_base", "con_base", "var_base", "sample_detections",
                                  "sample_5x_detections", "DivergentSite_count", "SNS_count", "SNV_count", "con_SNV_count", "pop_SNV_count",
                                  "sample_con_bases"]
    assert info.index.tolist() == list(range(len(golden["pm"]))) and info["position"].tolist() == golden["pm"].index.tolist()
    for c in golden["pm"].columns:
        assert info[c].astype(object).tolist() == golden["pm"][c].astype(object).tolist(), c
    assert "position" not in golden["pm"].columns                # (the caller's frame is left alone)
    assert len(compare.pooled_SNV_info(golden["pm"].iloc[:0])) == 0


def test_pooled_SNV_data_round_trip(golden):
    dst = golden["dst"]
    samples = [s for s, *_ in golden["samples"]]
    data, keys = compare.pooled_SNV_data(dst, samples=samples)
    assert list(data.columns) == ["sample", "scaffold", "position", "A", "C", "T", "G"] and list(keys.columns) == ["key", "sample", "scaffold"]
    assert data["sample"].dtype.kind == "i" and data["scaffold"].dtype.kind == "i" and data.index.tolist() == list(range(len(dst)))
    # numbered in the set's order; a key that names no scaffold / no sample is NaN there
    assert keys["key"].tolist() == [0, 1, 2, 3] and keys["sample"].tolist() == samples and keys["scaffold"].tolist() == ["a", "d", "e", "f"]
    back = pd.DataFrame({c: data[c].to_numpy() for c in "ACTG"},
                        index=pd.MultiIndex.from_arrays([data["sample"].map(keys.set_index("key")["sample"]).to_numpy(), data["position"].to_numpy()]))
    back["scaffold"] = pd.Categorical(data["scaffold"].map(keys.set_index("key")["scaffold"]), dtype=dst["scaffold"].dtype)
    pool_ref.same_frames(back, dst)
    one = dst[dst["scaffold"] == "a"].copy()
    one["scaffold"] = one["scaffold"].cat.remove_unused_categories()
    data, keys = compare.pooled_SNV_data(one)
    assert keys["scaffold"].isna().tolist() == [False, True, True, True] and keys["sample"].tolist() == samples


class RecordingPool:
    def __init__(self, events):
        self.events = events

    def pool_add(self, sample_name, batch, batch_scaffold_names, batch_bounds):
        self.events.append(("pool", sample_name, batch, tuple(batch_scaffold_names), tuple(int(x) for x in batch_bounds)))


@pytest.fixture
def stand_in_splits(monkeypatch):
    monkeypatch.setattr(pu, "tables_to_splits", lambda res, bounds, s_scaff, s_num, *a, **kw:
                        [types.SimpleNamespace(scaffold=n, split_number=i) for n, i in zip(s_scaff, s_num)])


def test_profile_bam_hook_pulls_every_batch_before_release(stand_in_splits):
    sc = {"s%d" % i: (1000 + 10 * i, 50, 60) for i in range(5)}
    groups = [[0], [1, 2], [3, 4]]
    w = World(sc, 2)
    w.run.pool_set, w.run.pool_sample = RecordingPool(w.events), "sampleA"
    w.go(groups, (4000, 500, 64))
    pulls = [e for e in w.events if e[0] == "pool"]
    assert len(pulls) == len(groups) == len(w.of("collect")) and w.logs == []
    names = list(sc)
    for pull, items in zip(pulls, groups):
        assert pull[1] == "sampleA" and pull[2] is None                                 # (the stand-in pipe's slot)
        assert pull[3] == tuple(names[k] for k in items)
        assert pull[4] == tuple(np.r_[0, np.cumsum([sc[names[k]][0] for k in items])].tolist())
    for t in (e[2] for e in w.of("collect")):                                           # collected, pulled, only then released
        i_c, i_r = w.events.index(("collect", 0, t)), w.events.index(("release", 0, t))
        assert len([e for e in w.events[i_c + 1:i_r] if e[0] == "pool"]) == 1
    # without the kwarg no such call is made
    w = World(sc, 2).go(groups, (4000, 500, 64))
    assert w.run.pool_set is None and not [e for e in w.events if e[0] == "pool"]


def test_a_pooling_run_with_one_mm_bin_asks_for_the_count_table(monkeypatch):
    made = []
    monkeypatch.setattr(pu.engine, "Pipe", lambda ctx, **kw: made.append(kw) or types.SimpleNamespace())
    opt = pu.profile_options({})
    for n_mm, pool in ((1, True), (4, True), (1, False), (4, False)):
        pu.open_pipe(None, opt, n_mm, 1, (100, 100, 4), **({"pool": True} if pool else {}))
    assert [bool(kw["want_counts"]) for kw in made] == [True, False, False, False]


def test_binding_declares_the_pool_entry_points():
    for f in ("enable", "sites", "fetch_sites", "add", "summary", "fetch_sample"):
        assert "isx_cmpset_pool_" + f in _lib.SYMBOLS
    assert _lib.POOL_SITE_DT.itemsize == 64 and _lib.ABI_VERSION == 5
