#!/usr/bin/env python3
"""tests/golden/make_pool_stored_golden.py -- the STORED inputs of SNV pooling (`inStrain compare -i IS1 IS2 ... --bams`).

Runs ONLY in the build container (needs the reference checkout).  The four samples over six scaffolds of make_pool_golden.py, by that
script's own construction: the script is imported (nothing is restated; the fixtures it stores on import are put back byte for
byte), with make_golden.run_reference_split watched, so that what the reference's profile_split machinery made for every (sample,
scaffold) is at hand:
  pool_stored_<sample>_snv.csv    the sample's cumulative_snv_table (every row the reference made: all mm, cryptic rows included)
  pool_stored_<sample>_covT.npz   its covT: scaffold, mm, positions, values -- one entry of each per (scaffold, mm) series, concatenated
                                  (series_scaffold, series_mm, series_offsets, positions, values)
Asserted: the saved tables are those PoolController.__init__ consumed -- without the cryptic rows and with the highest mm of every
(scaffold, position) they are that script's `own` tables.  Only data is stored.

usage: python tests/golden/make_pool_stored_golden.py
"""
import os
import sys

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                                        # noqa: E402

made = []                                                       # (scaffold, covT, SNV table) in the order of the calls
_run = mg.run_reference_split


def watched(mods, scaffold, *a, **k):
    res = _run(mods, scaffold, *a, **k)
    made.append((scaffold, res[0], res[2]))
    return res


mg.run_reference_split = watched
# the neighbour stores its fixtures when it is imported (npz members carry the time of writing): they are put back byte for byte
FIXTURES = [os.path.join(HERE, f) for f in ("pool_obs.npz", "pool_DSTdb.csv", "pool_PMdb.csv")]
kept = {f: open(f, "rb").read() for f in FIXTURES}
try:
    import make_pool_golden as mpg                              # noqa: E402  (its module body IS the construction, asserts included)
finally:
    mg.run_reference_split = _run
    for f, data in kept.items():
        with open(f, "wb") as out:
            out.write(data)
SAMPLES, NAMES, tables, cols, own = mpg.SAMPLES, mpg.NAMES, mpg.tables, mpg.cols, mpg.own

calls = iter(made)
for s in SAMPLES:
    sc_, mm_, off, pos, val = [], [], [0], [], []
    for name in NAMES:
        if (s, name) not in cols:
            continue
        scaffold, covT, S = next(calls)
        assert scaffold == name
        for mm in sorted(covT):
            ser = covT[mm]
            sc_.append(name); mm_.append(int(mm))
            pos.append(ser.index.to_numpy().astype(np.int64)); val.append(ser.to_numpy().astype(np.int64))
            off.append(off[-1] + len(ser))
    table = tables[s]
    # what PoolController.__init__ does with the stored table (polymorpher.py:53-70) gives the own rows the golden tables came from
    t = table[table["cryptic"] == False]                        # noqa: E712
    t = t.sort_values("mm").drop_duplicates(subset=["scaffold", "position"], keep="last").sort_index()
    o = own[s]
    key = ["scaffold", "position"]
    a = t.sort_values(key).reset_index(drop=True)
    b = o.sort_values(key).reset_index(drop=True)
    shared = [c for c in b.columns if c in a.columns]           # (the controller drops the columns it has no use for)
    assert set(key + ["A", "C", "T", "G", "class", "con_base"]) <= set(shared), shared
    assert len(a) == len(b) and all(a[c].astype(object).tolist() == b[c].astype(object).tolist() for c in shared), s
    np.savez_compressed(os.path.join(HERE, "pool_stored_%s_covT.npz" % s), series_scaffold=np.array(sc_), series_mm=np.array(mm_, np.int32),
                        series_offsets=np.array(off, np.int64), positions=np.concatenate(pos + [np.zeros(0, np.int64)]),
                        values=np.concatenate(val + [np.zeros(0, np.int64)]))
    table.to_csv(os.path.join(HERE, "pool_stored_%s_snv.csv" % s), index=False)
    print(s, len(table), "SNV rows,", int((table["cryptic"] == True).sum()), "cryptic,", len(sc_), "covT series")   # noqa: E712
assert next(calls, None) is None
