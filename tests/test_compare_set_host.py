"""CPU-only: the host side of the comparison set (instrain_amd/compare.py SampleSet / genome_wide): the set's word-aligned position
space and the pair kernel's tile directory (isx_cmpset_layout / isx_cmpset_tiles), the level axis (isx_cmpset_level_map), the
genome-level roll-up against the reference's own _add_stb + _genome_wide_readComparer (tests/golden/make_compare_genome_golden.py),
and profile_bam's hook that adds every collected batch to a set before its slot is released."""
import json
import os
import types

import numpy as np
import pandas as pd
import pytest

from instrain_amd import _lib, compare
from instrain_amd.profile import profile_utilities as pu
from tests.test_profile_driver_host import World

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LENGTHS = [1, 63, 64, 65, 127, 128, 129, 5000]


def test_set_layout_offsets_and_pad():
    off = compare.set_layout(LENGTHS)
    assert off.tolist() == [0, 1, 2, 3, 5, 7, 9, 12, 12 + 79]
    words = np.diff(off)
    pad = words * 64 - np.array(LENGTHS)
    assert pad.tolist() == [63, 1, 0, 63, 1, 0, 63, 79 * 64 - 5000] and (pad >= 0).all() and (pad < 64).all()
    with pytest.raises(_lib.IsxError):
        compare.set_layout([10, 0, 5])
    with pytest.raises(_lib.IsxError):
        compare.set_layout([1 << 31, 1 << 31])                  # the padded space must stay below 2^32 positions


@pytest.mark.parametrize("tile_words", [1, 2, 3, 64, 78, 79, 1024])
def test_tile_directory_never_crosses_a_scaffold(tile_words):
    off = compare.set_layout(LENGTHS)
    tiles = compare.tile_directory(LENGTHS, tile_words)
    assert (tiles["n_words"] >= 1).all() and (tiles["n_words"] <= tile_words).all()
    at = 0
    for sc in range(len(LENGTHS)):
        mine = tiles[tiles["scaffold"] == sc]
        n_words = int(off[sc + 1] - off[sc])
        assert len(mine) == -(-n_words // tile_words)
        assert mine["word0"].tolist() == list(range(int(off[sc]), int(off[sc + 1]), tile_words))       # consecutive, from its first word
        assert (mine["word0"] + mine["n_words"] <= off[sc + 1]).all()                                  # no tile reaches the next scaffold
        assert int(mine["n_words"][-1]) == n_words - (len(mine) - 1) * tile_words                      # the last tile's length
        assert (mine["n_words"][:-1] == tile_words).all()
        assert (tiles["scaffold"][at:at + len(mine)] == sc).all()                                      # set order
        at += len(mine)
    assert at == len(tiles) and int(tiles["n_words"].sum()) == int(off[-1])
    with pytest.raises(_lib.IsxError):
        compare.tile_directory(LENGTHS, 0)


def test_level_axis_and_map():
    axis, lmap = compare.level_map([[0, 1, 3], [0, 2], [0], [], [2, 3]])
    assert axis.tolist() == [0, 1, 2, 3]
    assert lmap[0].tolist() == [0, 1, 1, 2]             # mm 2 is not its own: level 1 (mm 1) carries over
    assert lmap[1].tolist() == [0, 0, 1, 1]             # beyond its last level: carried over
    assert lmap[2].tolist() == [0, 0, 0, 0]             # a single-level sample
    assert lmap[3].tolist() == [-1, -1, -1, -1]         # a sample that was never added
    assert lmap[4].tolist() == [-1, -1, 0, 1]           # none yet below its first value
    axis, lmap = compare.level_map([[7]])
    assert axis.tolist() == [7] and lmap.tolist() == [[0]]
    with pytest.raises(_lib.IsxError) as e:             # refused, not clamped
        compare.level_map([[0, 1, 3], [0, 2]], cap_axis=3)
    assert e.value.code == _lib.ERR_CAPACITY
    for bad in ([[0, 0]], [[3, 1]], [[-1]], [[70000]]):
        with pytest.raises(_lib.IsxError):
            compare.level_map(bad)
    assert _lib.CMPSET_MAX_LEVELS == 128


@pytest.mark.parametrize("mm_level", [False, True])
def test_genome_wide_vs_reference(mm_level):
    table = pd.read_csv(os.path.join(GOLDEN, "compare_genome_table.csv"), float_precision="round_trip")
    inputs = json.load(open(os.path.join(GOLDEN, "compare_genome_inputs.json")))
    exp = pd.read_csv(os.path.join(GOLDEN, "compare_genome_golden_mm.csv" if mm_level else "compare_genome_golden.csv"), float_precision="round_trip")
    assert "free_1" in set(table["scaffold"]) and "free_1" not in inputs["stb"]                        # a scaffold the stb does not name
    for rows in (table, table.to_dict("records"), table.iloc[::-1]):
        got = compare.genome_wide(rows, inputs["stb"], inputs["bin2length"], mm_level=mm_level)
        assert list(got.columns) == list(exp.columns) and len(got) == len(exp)
        assert ("mm" in got.columns) == mm_level
        # n of the bound: the rows summed for a genome's row = its scaffolds that have a row of the pair (at a level <= mm)
        named = table.assign(genome=table["scaffold"].map(inputs["stb"])).dropna(subset=["genome"])
        mms = exp["mm"] if mm_level else [named["mm"].max()] * len(exp)
        n = np.array([named[(named["genome"] == a) & (named["name1"] == b) & (named["name2"] == d) & (named["mm"] <= m)]["scaffold"].nunique()
                      for a, b, d, m in zip(exp["genome"], exp["name1"], exp["name2"], mms)], dtype=np.float64)
        assert (n >= 1).all() and n.max() >= 3
        for c in exp.columns:
            if exp[c].dtype.kind in "iO":
                assert got[c].tolist() == exp[c].tolist(), c
                continue
            g, e = got[c].to_numpy(np.float64), exp[c].to_numpy(np.float64)
            assert (np.isnan(g) == np.isnan(e)).all(), c
            ok = ~np.isnan(e)
            assert (np.abs(g[ok] - e[ok]) <= (n[ok] + 1) * 2.0 ** -52 * np.abs(e[ok])).all(), c
    z = exp[exp["genome"] == "gZ"]
    assert len(z) and z["coverage_overlap"].isna().all() and z["popANI"].isna().all() and (z["compared_bases_count"] == 0).all()
    assert table[(table["scaffold"] == "gA_3")]["popANI"].isna().any()                                  # a NaN ANI row inside gA
    # without bin2length there is no percent_compared; nothing to roll up -> None, as _add_stb
    assert "percent_compared" not in compare.genome_wide(table, inputs["stb"], None, mm_level=mm_level).columns
    assert compare.genome_wide([], inputs["stb"]) is None and compare.genome_wide(table, {"elsewhere": "g"}) is None


class RecordingSet:
    def __init__(self, events):
        self.events = events

    def add_batch(self, sample_name, batch, batch_scaffold_names, batch_bounds, mm_values=None):
        self.events.append(("add", sample_name, batch, tuple(batch_scaffold_names), tuple(int(x) for x in batch_bounds), mm_values))


@pytest.fixture
def stand_in_splits(monkeypatch):
    monkeypatch.setattr(pu, "tables_to_splits", lambda res, bounds, s_scaff, s_num, *a, **kw:
                        [types.SimpleNamespace(scaffold=n, split_number=i) for n, i in zip(s_scaff, s_num)])


def test_profile_bam_hook_adds_every_batch_before_release(stand_in_splits):
    sc = {"s%d" % i: (1000 + 10 * i, 50, 60) for i in range(5)}
    groups = [[0], [1, 2], [3, 4]]
    w = World(sc, 2)
    w.run.compare_set, w.run.compare_sample, w.run.mm_values = RecordingSet(w.events), "sampleA", np.array([0, 2, 5])
    w.go(groups, (4000, 500, 64))
    adds = [e for e in w.events if e[0] == "add"]
    assert len(adds) == len(groups) == len(w.of("collect")) and w.logs == []
    names = list(sc)
    for add, items in zip(adds, groups):
        assert add[1] == "sampleA" and add[2] is None                                   # (the stand-in pipe's slot)
        assert add[3] == tuple(names[k] for k in items)
        assert add[4] == tuple(np.r_[0, np.cumsum([sc[names[k]][0] for k in items])].tolist())
        assert add[5] is w.run.mm_values
    for t in (e[2] for e in w.of("collect")):                                           # collected, added, only then released
        i_c, i_r = w.events.index(("collect", 0, t)), w.events.index(("release", 0, t))
        between = [e for e in w.events[i_c + 1:i_r] if e[0] == "add"]
        assert len(between) == 1 and between[0][3] == tuple(names[k] for k in w.tids_of[t])
    # a failing add is the batch's failure: its slot is still released, the group is then run scaffold by scaffold
    w = World(sc, 1)

    class Refusing(RecordingSet):
        def add_batch(self, *a, **kw):
            super().add_batch(*a, **kw)
            if len([e for e in self.events if e[0] == "add"]) == 1:
                raise _lib.IsxError(-6, "added before")
    w.run.compare_set, w.run.compare_sample = Refusing(w.events), "sampleA"
    w.go([[0, 1]], (4000, 500, 64))
    assert sorted(e[2] for e in w.of("release")) == sorted(e[2] for e in w.of("submit")) and not w.pipes[0].open_tickets


def test_profile_bam_without_the_kwarg_adds_nothing(stand_in_splits):
    sc = {"s%d" % i: (1000 + 10 * i, 50, 60) for i in range(3)}
    w = World(sc, 2).go([[0], [1, 2]], (4000, 500, 64))
    assert w.run.compare_set is None and not [e for e in w.events if e[0] == "add"]
    assert len(w.of("collect")) == 2 and sorted(w.out) == sorted("%s.%d" % (n, i) for n in sc for i in (0, 1))
