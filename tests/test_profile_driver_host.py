"""CPU-only: profile_bam's planning steps and its batch driver (profile_utilities._BatchRun) with stand-ins for the pipe and the BAM
handle -- the in-flight window, the growth of a pipe that is too small, the scaffold-by-scaffold fallback and the failure lines."""
import types
from concurrent.futures import Future

import numpy as np
import pandas as pd
import pytest

from instrain_amd import _lib
from instrain_amd.profile import profile_utilities as pu

NEVER = 10 ** 12                                    # a segment count no pipe holds


class FakeBam:
    """segs: tid -> the segments its reads really are; info["n_segs"] after a submit = that count, or `reports` when given"""

    def __init__(self, segs, reports=None):
        self.segs, self.reports, self.info = segs, reports, {}


class FakePipe:
    """refuses a batch of more segments than it was made for, and any ticket it did not issue or any call after close()"""

    def __init__(self, world, seg_cap):
        self.world, self.seg_cap, self.closed = world, seg_cap, False
        self.no = len(world.pipes)
        self.open_tickets = set()
        world.pipes.append(self)

    def submit_bam(self, bf, tids, ref, bounds, **kw):
        assert not self.closed and len(ref) == bounds[-1]
        n = sum(bf.segs[t] for t in tids)
        bf.info = {"n_segs": n if bf.reports is None else bf.reports}
        if n > self.seg_cap:
            raise _lib.IsxError(_lib.ERR_CAPACITY, "more segments than the pipe's capacity")
        t = self.world.next_ticket = self.world.next_ticket + 1
        self.open_tickets.add(t)
        self.world.tids_of[t] = tuple(tids)
        self.world.events.append(("submit", self.no, t))
        self.world.most_out = max(self.world.most_out, sum(len(p.open_tickets) for p in self.world.pipes))
        return t

    def collect(self, t, **kw):
        if self.closed or t not in self.open_tickets:
            raise AssertionError("ticket %d collected on a pipe that does not hold it" % t)
        self.world.events.append(("collect", self.no, t))
        if self.world.tids_of[t] in self.world.bad_batches:
            self.world.bad_batches.remove(self.world.tids_of[t])
            raise RuntimeError("the device batch failed")
        return {"slot": None}

    def release(self, t):
        if self.closed or t not in self.open_tickets:
            raise AssertionError("ticket %d released on a pipe that does not hold it" % t)
        self.open_tickets.remove(t)
        self.world.events.append(("release", self.no, t))

    def close(self):
        assert not self.open_tickets, "a pipe closed with tickets out"
        self.closed = True
        self.world.events.append(("close", self.no))


class World:
    """a run's stand-ins: scaffolds `name -> (length, real segments, estimated segments)` in header order, two splits each"""

    def __init__(self, scaffolds, depth, reports=None, bad_batches=()):
        self.pipes, self.events, self.caps, self.tids_of = [], [], [], {}
        self.next_ticket = self.most_out = 0
        self.bad_batches = list(bad_batches)
        names = list(scaffolds)
        self.refs = [(n, scaffolds[n][0], None) for n in names]
        self.plan = [(t, n, [(0, 0, scaffolds[n][0] // 2 - 1), (1, scaffolds[n][0] // 2, scaffolds[n][0] - 1)]) for t, n in enumerate(names)]
        self.bf = FakeBam({t: scaffolds[n][1] for t, n in enumerate(names)}, reports)
        self.logs, self.out = [], {}
        codes = []
        for n in names:
            f = Future()
            f.set_result(np.zeros(scaffolds[n][0], dtype=np.uint8))
            codes.append(f)
        self.run = pu._BatchRun(self.bf, self.plan, self.refs, pu.profile_options({}), self.make_pipe, depth, codes,
                                [scaffolds[n][2] for n in names], self.out, pu._StageClock(None), bam="x.bam", logs=self.logs)

    def make_pipe(self, need):
        self.caps.append(need)
        return FakePipe(self, need[1])

    def go(self, item_groups, need):
        self.run.open_pipe(need)
        layouts = []
        for items in item_groups:
            f = Future()
            f.set_result(self.run.layout(items))
            layouts.append(f)
        self.run.run(item_groups, layouts)
        assert layouts == [None] * len(item_groups) or self.logs
        return self

    def of(self, kind):
        return [e for e in self.events if e[0] == kind]


@pytest.fixture(autouse=True)
def stand_in_splits(monkeypatch):
    made = []

    def fake_tables_to_splits(res, bounds, s_scaff, s_num, s_off, s_len, min_freq, bam_name=None, **kw):
        made.extend(zip(s_scaff, s_num))
        return [types.SimpleNamespace(scaffold=n, split_number=i) for n, i in zip(s_scaff, s_num)]
    monkeypatch.setattr(pu, "tables_to_splits", fake_tables_to_splits)
    return made


def _keys(names):
    return sorted("%s.%d" % (n, i) for n in names for i in (0, 1))


def test_window_of_batches_in_flight(stand_in_splits):
    """depth d, n > d groups: never more than d tickets out, collected in submission order, each released once, every split in out"""
    sc = {"s%d" % i: (1000 + 10 * i, 50, 60) for i in range(7)}
    for depth in (1, 2, 3):
        w = World(sc, depth).go([[0], [1, 2], [3], [4], [5], [6]], (4000, 500, 64))
        assert w.most_out == depth
        tickets = [e[2] for e in w.of("submit")]
        assert len(tickets) == 6 and [e[2] for e in w.of("collect")] == tickets and sorted(e[2] for e in w.of("release")) == sorted(tickets)
        assert sorted(w.out) == _keys(sc) and w.logs == [] and w.caps == [(4000, 500, 64)]
        assert not w.pipes[0].open_tickets and not w.run.in_flight
    assert len(stand_in_splits) == 3 * 14


def test_a_short_estimate_rebuilds_the_pipe_once():
    """a group of 5 x the pipe's segment capacity S: the batches in flight come home before the old pipe goes, ONE rebuild for
    max(2 S, n + 4096) segments, and that is the capacity the run goes on with"""
    S = 1000
    sc = {"a": (1000, 10, 10), "b": (1200, 10, 10), "big": (3000, 5 * S, 10), "c": (900, 10, 10)}
    w = World(sc, 3).go([[0], [1], [2], [3]], (2000, S, 64))
    assert [c[1] for c in w.caps] == [S, max(2 * S, 5 * S + 4096)]
    assert w.caps[1] == (3000, 5 * S + 4096, 64) and w.run.cap == w.caps[1]        # positions / splits never below the floor
    close = w.events.index(("close", 0))
    assert [e[:2] for e in w.events[:close]].count(("release", 0)) == 2             # a and b were collected on the pipe that issued them
    assert all(e[1] == 1 for e in w.events[close + 1:])
    assert sorted(w.out) == _keys(sc) and w.logs == []


def test_growth_factors_apply_to_the_base_not_to_the_grown_value():
    """the front end reports few segments and nothing below 6 S fits: 2 S, then 8 S -- not 4 x the first retry's 2 S"""
    S = 10_000
    sc = {"a": (1000, 10, 10), "big": (3000, 6 * S, 10)}
    w = World(sc, 2, reports=10).go([[0], [1]], (3000, S, 64))
    assert [c[1] for c in w.caps] == [S, 2 * S, 8 * S]
    assert sorted(w.out) == _keys(sc) and w.logs == []
    # a first retry sized by the front end's count (2 S + 4096 > 2 S) is not what the second one multiplies
    w = World(sc, 2, reports=2 * S).go([[0], [1]], (3000, S, 64))
    assert [c[1] for c in w.caps] == [S, 2 * S + 4096, 8 * S]
    assert sorted(w.out) == _keys(sc) and w.logs == []


def test_a_group_that_never_fits_goes_scaffold_by_scaffold():
    """three rebuilt pipes (2, 8, 32 x the same base), then every scaffold alone: the one that fits no pipe is dropped with one failure
    line per split, the others of its group are profiled"""
    S, est = 5000, 7000
    sc = {"a": (1000, 10, 10), "never": (3000, NEVER, est), "c": (900, 10, 10), "d": (800, 10, 10)}
    w = World(sc, 2, reports=10).go([[0, 1, 2], [3]], (5000, S, 64))
    assert [c[1] for c in w.caps] == [S, 2 * S, 8 * S, 32 * S] + [2 * est, 8 * est, 32 * est]
    assert w.caps[4] == (3000, 2 * est, 3)                                           # alone: no floor but the scaffold's own size
    assert sorted(w.out) == _keys(["a", "c", "d"])
    assert len(w.logs) == 2 and all("FAILURE SplitException never %d" % i in line for i, line in enumerate(w.logs))
    assert [p.closed for p in w.pipes] == [True] * 6 + [False] and not w.pipes[-1].open_tickets


def test_a_failing_batch_in_the_middle_of_the_window(stand_in_splits):
    """collect fails for the second of three batches in flight: the third comes home on the pipe that issued its ticket before the
    failed group is run again scaffold by scaffold; no split is lost or made twice"""
    sc = {"a": (1000, 10, 10), "b": (1200, 10, 10), "c": (900, 10, 10), "d": (800, 10, 10)}
    w = World(sc, 3, bad_batches=[(1, 2)]).go([[0], [1, 2], [3]], (3000, 500, 64))
    assert w.of("collect")[:3] == [("collect", 0, 1), ("collect", 0, 2), ("collect", 0, 3)]
    again = [w.tids_of[e[2]] for e in w.of("submit")[3:]]
    assert again == [(1,), (2,)] and w.events.index(("release", 0, 3)) < w.events.index(("submit", 0, 4))
    assert sorted(e[2] for e in w.of("release")) == [1, 2, 3, 4, 5]
    assert sorted(w.out) == _keys(sc) and w.logs == [] and len(w.caps) == 1
    assert sorted(stand_in_splits) == sorted((n, i) for n in sc for i in (0, 1))


def test_select_scaffolds_failures_and_order():
    refs = [("ok0", 100, None), ("noseq", 50, None), ("ok1", 300, None), ("wronglen", 80, None), ("notile", 60, None)]
    s2s = {"ok0": "A" * 100, "ok1": "C" * 300, "wronglen": "A" * 79, "notile": "G" * 60, "missing": "ACGT"}
    rows = [("ok1", 0, 0, 149), ("ok1", 1, 150, 299), ("missing", 0, 0, 1), ("missing", 1, 2, 3), ("noseq", 0, 0, 49),
            ("wronglen", 0, 0, 29), ("wronglen", 1, 30, 59), ("wronglen", 2, 60, 79), ("notile", 0, 0, 29), ("notile", 1, 31, 59),
            ("ok0", 0, 0, 99)]
    fdb = pd.DataFrame(rows, columns=["scaffold", "split_number", "start", "end"])
    plan, failed = pu.select_scaffolds(refs, s2s, fdb, 10000, "x.bam")
    assert plan == [(0, "ok0", [(0, 0, 99)]), (2, "ok1", [(0, 0, 149), (1, 150, 299)])]          # header order, not the table's
    assert {n: (str(e), k) for n, (e, k) in failed.items()} == {
        "missing": ("scaffold missing is not in the .bam file x.bam!", 2),
        "noseq": ("scaffold noseq has no sequence / its length differs from the .bam header", 1),
        "wronglen": ("scaffold wronglen has no sequence / its length differs from the .bam header", 3),
        "notile": ("fasta_db splits of notile do not tile [0, 60)", 2)}
    assert all(isinstance(e, ValueError) for e, _ in failed.values())
    logs = []
    for name, (e, k) in failed.items():
        pu._fail(logs, name, range(k))
    assert len(logs) == 8 and sum("FAILURE SplitException wronglen 2" in line for line in logs) == 1
    # without a fasta_db: every reference that has a sequence, iterate_splits' windows
    plan, failed = pu.select_scaffolds(refs, s2s, None, 200, "x.bam")
    assert [(t, n) for t, n, _ in plan] == [(0, "ok0"), (2, "ok1"), (4, "notile")]
    assert plan[1][2] == [(i, s, e) for i, (s, e) in enumerate(pu.iterate_splits(300, 200))] and len(plan[1][2]) == 2
    assert list(failed) == ["wronglen"] and failed["wronglen"][1] == 1


def test_options_are_parsed_once_with_todays_defaults():
    o = pu.profile_options({})
    assert (o.window_length, o.skip_mm, o.min_cov, o.min_freq, o.min_snp, o.rarefied, o.seed) == (10000, False, 5, .05, 10, 50, 0)
    assert (o.store_everything, o.strict, o.host_threads, o.scan_threads) == (False, False, 0, 0)
    assert (o.batch_positions, o.batch_segs, o.pipe_depth, o.layout, o.jump_slack) == (64_000_000, 4_000_000, None, None, None)
    assert o.filter == dict(min_read_ani=0.95, min_mapq=-1, max_insert_relative=3, min_insert=50, pairing_filter='paired_only')
    assert o.filter == pu.read_filter_flags({})
    assert pu.pipe_depth_of(o, 1) == 1 and pu.pipe_depth_of(o, 2) == 2
    assert pu.profile_options(dict(batch_observations=10_000)).batch_segs == max(64, 10_000 // 150) == 66
    assert pu.profile_options(dict(batch_observations=1_000)).batch_segs == 64
    assert pu.profile_options(dict(batch_observations=10_000, batch_reads=77)).batch_segs == 77
    o = pu.profile_options(dict(host_threads=8, pipe_depth=0, min_read_ani=0.9, skip_mm_profiling=1, strict=1))
    assert (o.scan_threads, o.skip_mm, o.strict, o.filter['min_read_ani']) == (8, True, True, 0.9)
    assert pu.pipe_depth_of(o, 5) == 1
    assert pu.profile_options(dict(host_threads=8, scan_threads=16)).scan_threads == 16


def test_split_table_and_segment_estimate():
    b, sc, num, off, ln, first = pu.split_table([("x", 250, [(0, 0, 99), (1, 100, 249)]), ("y", 40, [(0, 0, 39)])])
    assert (b, sc, num, off, ln, first) == ([0, 100, 250, 290], ["x", "x", "y"], [0, 1, 0], [0, 0, 250], [100, 150, 40], [0, 2, 3])
    plan = [(0, "x", []), (2, "y", [])]
    assert pu.estimate_segments({}, [100, 7, 8], plan) == [100 + 25 + 64, 10 + 64]                        # 150-base reads: 1.25 a read
    assert pu.estimate_segments({"filtered_pairs": 10, "filtered_bases": 10 * 2 * 224}, [100, 7, 8], plan) == [225 + 64, 18 + 64]
    assert pu.largest_need([[0], [1]], plan, [("x", 250, None), ("-", 9, None), ("y", 40, None)], [189, 74]) == (250, 189, 1)
