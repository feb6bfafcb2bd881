"""CPU: the host half of pooling from stored profiles (instrain_amd.compare): pack_profile(pool=True)'s flags against the reference's
stored tables (tests/golden/make_pool_stored_golden.py), its ValueErrors, pool_window's column arithmetic, and pool_stored's window
walk over a stand-in BAM and set."""
import os

import numpy as np
import pandas as pd
import pytest

from instrain_amd import compare, engine

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CLASSES = ["AmbiguousReference", "DivergentSite", "SNS", "SNV", "con_SNV", "pop_SNV"]
NAMES, LENGTHS = ["a", "b", "c", "d", "e", "f"], [1, 63, 64, 65, 129, 300]
INDEX = {n: i for i, n in enumerate(NAMES)}


def _golden(sample):
    z = np.load(os.path.join(GOLDEN, "pool_stored_%s_covT.npz" % sample))
    off, covT = z["series_offsets"], {}
    for k, (sc, mm) in enumerate(zip(z["series_scaffold"].tolist(), z["series_mm"].tolist())):
        covT.setdefault(str(sc), {})[int(mm)] = (z["positions"][off[k]:off[k + 1]], z["values"][off[k]:off[k + 1]])
    return covT, pd.read_csv(os.path.join(GOLDEN, "pool_stored_%s_snv.csv" % sample), keep_default_na=False)


@pytest.mark.parametrize("sample", ["s0", "s1", "s2", "s3"])
def test_flags_of_the_golden_tables(sample):
    covT, table = _golden(sample)
    p = compare.pack_profile(INDEX, LENGTHS, covT, table, pool=True)
    plain = compare.pack_profile(INDEX, LENGTHS, covT, table)
    assert "flags" not in plain and plain["snv"].tobytes() == p["snv"].tobytes() and len(p["flags"]) == len(p["snv"]) == len(table)
    assert p["flags"].dtype == np.uint8
    assert [CLASSES[f & 7] for f in p["flags"]] == table["class"].tolist()
    assert [bool(f & 8) for f in p["flags"]] == table["cryptic"].tolist() and not (p["flags"] & 0xF0).any()
    if sample == "s0":
        assert (p["flags"] & 8).any() and len(set((p["flags"] & 7).tolist())) > 1
    # rows of scaffolds the set does not name are dropped together with their flags
    sub = compare.pack_profile({"f": 0}, [300], covT, table, pool=True)
    assert len(sub["flags"]) == len(sub["snv"]) == int((table["scaffold"] == "f").sum())
    assert [CLASSES[f & 7] for f in sub["flags"]] == table[table["scaffold"] == "f"]["class"].tolist()


def test_pack_profile_pool_value_errors():
    covT, table = _golden("s0")
    for col in ("class", "cryptic"):
        with pytest.raises(ValueError, match=col):
            compare.pack_profile(INDEX, LENGTHS, covT, table.drop(columns=[col]), pool=True)
    odd = table.copy()
    odd.loc[odd.index[0], "class"] = "nonsense_SNV"
    with pytest.raises(ValueError, match="class"):
        compare.pack_profile(INDEX, LENGTHS, covT, odd, pool=True)
    odd = table.copy()
    odd["cryptic"] = 2
    with pytest.raises(ValueError, match="cryptic"):
        compare.pack_profile(INDEX, LENGTHS, covT, odd, pool=True)
    compare.pack_profile(INDEX, LENGTHS, covT, table.drop(columns=["class", "cryptic"]))          # without pooling nothing is asked of them
    assert len(compare.pack_profile(INDEX, LENGTHS, covT, None, pool=True)["flags"]) == 0


def test_pool_window_arithmetic():
    assert compare.pool_window([0, 5, 9], [False, True, False]) == (0, 10, 2)                      # a site at position 0: lo stays 0
    assert compare.pool_window([3, 5, 299], [False, False, False]) == (2, 300, 3)                  # the last position of a 300-long scaffold
    assert compare.pool_window([3, 5, 299], [True, False, True]) == (4, 6, 1)                      # owned sites do not widen the window
    assert compare.pool_window([0], [False]) == (0, 1, 1)
    assert compare.pool_window([7, 8], [True, True]) is None and compare.pool_window([], []) is None


class _Set:
    """what pool_stored asks of a SampleSet"""

    def __init__(self, plans):
        self.plans, self.columns, self.done = plans, {}, []

    def pool_plan(self, name):
        return dict(self.plans[name])

    def pool_add_obs(self, name, scaffolds, obs, offsets, gpos0=None):
        assert len(scaffolds) == 1 and list(offsets) == [0, len(obs)] and gpos0 is None
        self.columns.setdefault((name, scaffolds[0]), []).extend(np.unique(obs["gpos"]).tolist())
        self.calls = getattr(self, "calls", 0) + 1
        return 0.5

    def pool_obs_done(self, name, scaffolds=None):
        self.done.append((name, list(scaffolds)))


class _Bam:
    """a BAM of two references with `depth` observations in every column"""
    opened, log = [], []

    def __init__(self, path):
        self.path, self.depth = path, 7
        _Bam.opened.append(path)

    def refs(self):
        return [("x", 1000, 0), ("y", 50, 1000)]

    def scan(self):
        _Bam.log.append("scan")

    def filter(self, **kw):
        _Bam.log.append(("filter", kw["min_read_ani"]))

    def set_r2m(self, tid, names, mm=None):
        _Bam.log.append(("r2m", tid, sorted(names)))

    def expand_region(self, tid, start, stop, copy=True, **kw):
        assert kw["skip_mm"] and not copy and 0 <= start < stop <= self.refs()[tid][1]
        obs = np.zeros((stop - start) * self.depth, dtype=engine.OBS_DT)
        obs["gpos"] = np.repeat(np.arange(start, stop), self.depth)
        return obs, None, None, None

    def close(self):
        _Bam.log.append("close")


def test_pool_stored_window_walk(monkeypatch):
    monkeypatch.setattr(engine, "BamFile", _Bam)
    _Bam.opened, _Bam.log = [], []
    plans = {"s": {"x": (10, 1000, 40), "y": (0, 50, 3)}, "t": {"y": (49, 50, 1)}, "u": {}}
    st = _Set(plans)
    out = compare.pool_stored(st, {"s": "s.bam", "t": "t.bam", "u": "u.bam"}, name2r2m={"s": {"y": {"p1": 0, "p0": 2}}, "t": {"y": None}},
                              max_obs=7 * 100, min_read_ani=0.9)
    # no column handed twice, none left out
    for (name, scaffold), cols in st.columns.items():
        lo, hi, _ = plans[name][scaffold]
        assert cols == list(range(lo, hi)), (name, scaffold)
    assert set(st.columns) == {("s", "x"), ("s", "y"), ("t", "y")}
    assert st.done == [("s", ["x", "y"]), ("t", ["y"]), ("u", [])]                                  # once per sample
    assert _Bam.opened == ["s.bam", "t.bam", "u.bam"] and _Bam.log.count("scan") == 3 == _Bam.log.count("close")
    # 990 columns of 7 with at most 700 observations a window: the dropped first window says 100 columns, then 10 windows; y goes at once
    assert out["s"] == {"scaffolds": 2, "windows": 11, "observations": 7 * (990 + 50), "device_ms": 0.5 * 11}
    assert out["t"]["windows"] == 1 and out["t"]["observations"] == 7 and out["u"] == {"scaffolds": 0, "windows": 0, "observations": 0, "device_ms": 0.0}
    assert ("filter", 0.9) in _Bam.log and ("r2m", 1, ["p0", "p1"]) in _Bam.log
    assert _Bam.log.count(("filter", 0.9)) == 2                                                      # s (for x) and t; u has nothing to pull
    with pytest.raises(ValueError, match="scaffold z is not in the .bam file s.bam"):
        compare.pool_stored(_Set({"s": {"z": (0, 5, 1)}}), {"s": "s.bam"})
    assert _Bam.log[-1] == "close"
