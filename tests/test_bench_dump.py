"""bench.py --dump-outputs on the host: OutputDump reads coverage and clonality over its sampled blocks straight from every shrunk
hand-back form a pipe slot may carry (16-bit, 8-bit, the lean 4-bit plane with 16-bit window rows; saturated list; sparse clonality)
and agrees with the library's own densifiers (engine.dense_cov / dense_clon); what it writes is finite float32 / float64 only."""
import os

import numpy as np

import bench
from instrain_amd import _lib, engine


def _forms(seed=0, n_pos=100_003, W=64):
    rng = np.random.default_rng(seed)
    true = rng.integers(0, 40, n_pos).astype(np.int64)
    true[rng.integers(0, n_pos, 50)] = 70_000                       # beyond 16 bits: only the saturated list holds them
    g = np.flatnonzero(true > 65534)
    sat = np.zeros(len(g), _lib.SAT_DT)
    sat["gpos"], sat["coverage"] = g, true[g]
    rng.shuffle(sat)                                                # (unordered, include/instrain_amd.h)
    nib = np.zeros((n_pos + 1) // 2 * 2, np.uint8)
    nib[:n_pos] = np.minimum(true, 15)
    wins = np.unique(np.flatnonzero(true >= 15) // W)
    rows = np.zeros((len(wins), W), np.uint16)
    for k, w in enumerate(wins):
        seg = true[w * W:(w + 1) * W]
        rows[k, :len(seg)] = np.minimum(seg, 65535)
    perm = rng.permutation(len(wins))                               # rows in no particular order
    cg = np.sort(rng.choice(np.flatnonzero(true >= 5), 500, replace=False))
    cs = np.zeros(len(cg), _lib.CLON_DT)
    cs["gpos"], cs["clon"] = cg, rng.random(len(cg)).astype(np.float32)
    forms = {"cov4": {"cov4": (nib[0::2] | (nib[1::2] << 4)).astype(np.uint8), "cov_window": W, "cov_row_win": wins[perm].astype(np.uint32),
                      "cov_rows": rows[perm], "saturated": sat, "clon_sparse": cs},
             "cov16": {"cov16": np.minimum(true, 65535).astype(np.uint16), "saturated": sat, "clon_sparse": cs},
             "cov8": {"cov8": np.minimum(true, 255).astype(np.uint8), "saturated": sat, "clon_sparse": cs}}
    return true, cs, forms


def test_dump_reads_every_coverage_form():
    true, cs, forms = _forms()
    n_pos = len(true)
    d = bench.OutputDump([{"n_pos": 10 ** 8}] * 25, min_cov=5)       # a sample of the headline's shape: a few whole blocks a batch
    at = d.positions(3)
    assert 0 < len(at) <= (1 << 18) // 25 and (np.diff(at) > 0).all() and at.max() < 10 ** 8
    for name, r in forms.items():
        d = bench.OutputDump([{"n_pos": n_pos}], min_cov=5)
        at = d.positions(0)
        cov, clon = d._coverage(r, 0)
        assert (cov == true[at]).all() and (cov > 65535).any(), name
        assert (np.minimum(cov, 65535) == engine.dense_cov(dict(r), n_pos)[at]).all(), name
        assert np.array_equal(clon, engine.dense_clon(np.minimum(true, 65535), cs, 5)[at], equal_nan=True), name


def test_dump_files(tmp_path):
    true, cs, forms = _forms(seed=1)
    rng = np.random.default_rng(2)
    snv = np.zeros(3000, _lib.SNV_DT)
    snv["gpos"] = np.sort(rng.choice(len(true), 3000, replace=False))
    snv["cnt"] = rng.integers(0, 9, (3000, 4))
    ld = np.zeros(40, _lib.LD_DT)
    ld["r2"] = rng.random(40)
    ws = [{"n_pos": len(true)}, {"n_pos": len(true)}]
    written = []
    for k in range(2):                                              # the same hand-back twice -> the same files
        d = bench.OutputDump(ws, min_cov=5)
        for i in range(2):
            d(i, dict(forms["cov4"], snv=snv, ld=ld, sizes={"n_snv": 3000, "n_ld": 40, "n_edges": 7}, rows_checksum=(1 << 63) + 12345))
        out = tmp_path / str(k)
        info = d.write(str(out))
        written.append({f[:-4]: np.load(str(out / f)) for f in os.listdir(str(out))})
        assert info["files"] == len(written[-1]) and info["bytes"] == sum(v.nbytes for v in written[-1].values())
    a, b = written
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and np.isfinite(a[k]).all(), k
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    # clonality: the defined values and the rows of coverage_position they belong to -- NaN (below min_cov) everywhere else
    d = bench.OutputDump(ws, min_cov=5)
    clon = np.full(len(a["coverage_position"]), np.nan, np.float32)
    clon[a["clonality_row"].astype(np.int64)] = a["clonality"]
    exp = engine.dense_clon(np.minimum(true, 65535), cs, 5)
    assert np.array_equal(clon, np.concatenate([exp[d.positions(i)] for i in range(2)]), equal_nan=True) and np.isnan(clon).any()
    assert (a["ld_r2_row"] == np.arange(80)).all()
    assert (a["batch_rows_checksum"] == [2.0 ** 31, 12345.0]).all() and (a["batch_rows"] == [3000, 40, 7]).all()
    assert a["snv_position"].dtype == np.float64 and a["snv_position"][3000:].min() >= len(true)      # flat over the pass
    assert len(a["snv_counts"]) == 6000 and len(a["ld_r2"]) == 80 and len(a["coverage"]) == len(a["coverage_position"])
