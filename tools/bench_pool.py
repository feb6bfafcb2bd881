#!/usr/bin/env python3
"""SNV pooling over a sample set (compare.SampleSet(pooling=True), isx_cmpset_pool_*) next to the host route the tree had before it:
  sites     SampleSet.pool_sites(): site plane, ranks, own rows scattered -- wall ms, the call waits for the device
  pull      SampleSet.pool_add() of one resident batch -- wall ms, median over the samples
  summary   isx_cmpset_pool_summary, event-timed device ms; tables = pooled_tables() wall ms (fetches + pandas)
  host      Batch.fetch()["counts"] per sample (16 bytes a position over the link; one-level leg only) + tests/pool_ref.pooled_tables on
            the same observations (oracle SNV call + pandas), wall ms; only up to --host-max samples
for S in --samples synthetic samples on two layouts: --genome-len positions with one level, --mm-genome-len positions with 6 levels
(--scaffolds scaffolds each).  Samples are --distinct different workloads over one reference, repeated.
python tools/bench_pool.py [--tag T]        --tag writes profiles/<T>_pool.md."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def leg(ctx, label, genome_len, coverage, skip_mm, S, args, lut, fb):
    from instrain_amd import compare, engine, synth
    from tests import pool_ref
    lens = [genome_len // args.scaffolds] * args.scaffolds
    lens[-1] += genome_len - sum(lens)
    sb = np.r_[0, np.cumsum(lens)].astype(np.int64)
    names = ["s%d" % i for i in range(args.scaffolds)]
    batches, works = [], []
    for k in range(min(S, args.distinct)):
        w = synth.make_workload(genome_len=genome_len, coverage=coverage, n_sites=genome_len // 1000, seed=11 + k, skip_mm=skip_mm, max_mm=5)
        if works:       # every workload brings its own random reference: the same differences on the first one's (a cyclic shift of the codes)
            at = w["obs"]["gpos"].astype(np.int64)
            w["obs"]["base"] = (w["obs"]["base"].astype(np.int64) - w["ref_codes"][at] + works[0]["ref_codes"][at]) % 4
            w["ref_codes"] = works[0]["ref_codes"]
        b = engine.Batch(ctx, w["ref_codes"], w["split_bounds"], w["obs"], w["pair"], n_mm_bins=int(w["n_mm_bins"]), enable_linkage=False)
        b.run()
        batches.append(b)
        works.append(w)
    st = compare.SampleSet(ctx, names, lens, min_cov=5, pooling=True)
    for k in range(S):
        st.add_batch("sample%d" % k, batches[k % len(batches)], names, sb)
    t0 = time.perf_counter()
    n_sites = st.pool_sites()
    sites_ms = (time.perf_counter() - t0) * 1e3
    pull_ms = []
    for k in range(S):
        t0 = time.perf_counter()
        st.pool_add("sample%d" % k, batches[k % len(batches)], names, sb)
        pull_ms.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    dst, pm = st.pooled_tables()
    tables_ms = (time.perf_counter() - t0) * 1e3
    summary_ms = st.pool_device_ms
    st.close()
    host_fetch_ms = host_ref_ms = None
    if S <= args.host_max:
        if skip_mm:
            t0 = time.perf_counter()
            for k in range(S):
                batches[k % len(batches)].fetch()["counts"]
            host_fetch_ms = (time.perf_counter() - t0) * 1e3
        seq = "".join(np.array(list("ACTG"))[works[0]["ref_codes"]])
        obs = [("sample%d" % k, works[k % len(works)]["obs"]["gpos"].astype(np.int64), works[k % len(works)]["obs"]["base"],
                works[k % len(works)]["obs"]["mm"].astype(np.int64)) for k in range(S)]
        t0 = time.perf_counter()
        ref_dst, ref_pm = pool_ref.pooled_tables(obs, seq, names, lens, lut, fb)
        host_ref_ms = (time.perf_counter() - t0) * 1e3
        pool_ref.same_frames(dst, ref_dst)
        pool_ref.same_frames(pm, ref_pm)
    for b in batches:
        b.close()
    return {"leg": label, "n_pos": int(genome_len), "scaffolds": args.scaffolds, "samples": S, "sites": int(n_sites), "dst_rows": len(dst),
            "pool_MB": round(17 * n_sites * S / 1e6 + (int(sb[-1]) + 63 * args.scaffolds) / 8 / 1e6, 3),
            "sites_wall_ms": round(sites_ms, 2), "pull_wall_ms_median": round(float(np.median(pull_ms)), 3),
            "pull_wall_ms_first": round(pull_ms[0], 3), "summary_device_ms": round(summary_ms, 4), "tables_wall_ms": round(tables_ms, 2),
            "host_fetch_counts_ms": None if host_fetch_ms is None else round(host_fetch_ms, 2),
            "host_pool_ref_ms": None if host_ref_ms is None else round(host_ref_ms, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-len", type=int, default=2_000_000)
    ap.add_argument("--mm-genome-len", type=int, default=500_000)
    ap.add_argument("--samples", default="2,8,32")
    ap.add_argument("--scaffolds", type=int, default=50)
    ap.add_argument("--distinct", type=int, default=4, help="different synthetic samples made (and resident) per leg")
    ap.add_argument("--host-max", type=int, default=8, help="run the host route up to this many samples")
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    from instrain_amd import engine
    from tests import util
    ctx = engine.Context(0)
    lut, fb = util.load_lut()
    ctx.set_null_model(lut, fb)
    out = []
    for S in (int(x) for x in args.samples.split(",")):
        out.append(leg(ctx, "one_level", args.genome_len, 12, True, S, args, lut, fb))
        print(json.dumps(out[-1]), flush=True)
        out.append(leg(ctx, "six_levels", args.mm_genome_len, 20, False, S, args, lut, fb))
        print(json.dumps(out[-1]), flush=True)
    ctx.close()
    if args.tag:
        path = os.path.join(REPO, "profiles", "%s_pool.md" % args.tag)
        with open(path, "w") as f:
            f.write("# SNV pooling over a sample set next to the host route (tools/bench_pool.py)\n\n")
            f.write("sites / pull / tables: wall ms of SampleSet.pool_sites, pool_add (one resident batch) and pooled_tables (the calls wait for "
                    "the device); summary_device_ms: event-timed isx_cmpset_pool_summary; host_fetch_counts_ms: Batch.fetch()['counts'] of "
                    "every sample (one-level leg); host_pool_ref_ms: tests/pool_ref.pooled_tables on the same observations, whose tables "
                    "the device's were checked against (up to %d samples).  %d different synthetic samples per leg, repeated.  One run, "
                    "single calls.\n\n" % (args.host_max, args.distinct))
            keys = list(out[0].keys())
            f.write("| " + " | ".join(keys) + " |\n|" + "---|" * len(keys) + "\n")
            for r in out:
                f.write("| " + " | ".join(str(r[k]) for k in keys) + " |\n")
        print("wrote", path)


if __name__ == "__main__":
    main()
