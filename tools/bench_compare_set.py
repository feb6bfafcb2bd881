#!/usr/bin/env python3
"""The comparison set (compare.SampleSet, isx_cmpset_*) next to the pair loop it replaces, event-timed device ms:
  add      isx_cmpset_add of one resident batch (levels cumulated, planes packed, last SNV rows kept) -- wall ms, the call waits
  compare  isx_cmpset_compare: every pair in one pass over the sketches
  loop     compare.compare_scaffolds over the same pairs on resident batches (only where --loop-max samples' batches fit)
for S in --samples synthetic samples on two layouts: --genome-len positions with one level, --mm-genome-len positions with 6 levels
(--scaffolds scaffolds each).  Samples are --distinct different workloads, repeated: the counts do not matter to the time.
python tools/bench_compare_set.py [--tag r09]        --tag writes profiles/<tag>_compare_set.md."""
import argparse
import itertools
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def leg(ctx, label, genome_len, coverage, skip_mm, S, args):
    from instrain_amd import compare, engine, synth
    lens = [genome_len // args.scaffolds] * args.scaffolds
    lens[-1] += genome_len - sum(lens)
    sb = np.r_[0, np.cumsum(lens)].astype(np.int64)
    names = ["s%d" % i for i in range(args.scaffolds)]
    batches = []
    for k in range(min(S, args.distinct)):
        w = synth.make_workload(genome_len=genome_len, coverage=coverage, n_sites=genome_len // 1000, seed=11 + k, skip_mm=skip_mm,
                                max_mm=5)
        b = engine.Batch(ctx, w["ref_codes"], w["split_bounds"], w["obs"], w["pair"], n_mm_bins=int(w["n_mm_bins"]), enable_linkage=False)
        b.run()
        batches.append(b)
        del w
    st = compare.SampleSet(ctx, names, lens, min_cov=5)
    add_ms = []
    for k in range(S):
        t0 = time.perf_counter()
        st.add_batch("sample%d" % k, batches[k % len(batches)], names, sb)
        add_ms.append((time.perf_counter() - t0) * 1e3)
    cmp_ms = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        table = st.compare()
        cmp_ms.append((round(st.device_ms, 4), round((time.perf_counter() - t0) * 1e3, 2)))
    levels = st.levels
    n_pairs = S * (S - 1) // 2
    loop_ms = None
    if S <= args.loop_max:
        loop_ms = 0.0
        for i, j in itertools.combinations(range(S), 2):
            _, _, ms = compare.compare_scaffolds(batches[i % len(batches)], batches[j % len(batches)], sb, names)
            loop_ms += ms
    st.close()
    for b in batches:
        b.close()
    M = int(levels.shape[2])
    return {"leg": label, "n_pos": int(genome_len), "levels": M, "scaffolds": args.scaffolds, "samples": S, "pairs": n_pairs,
            "plane_MB_per_sample": round(M * (int(sb[-1]) + 63 * args.scaffolds) / 8 / 1e6, 2),
            "add_wall_ms_first": round(add_ms[0], 2), "add_wall_ms_median": round(float(np.median(add_ms)), 2),
            "compare_device_ms": [c[0] for c in cmp_ms], "compare_wall_ms": [c[1] for c in cmp_ms], "table_rows": len(table),
            "pair_loop_device_ms": None if loop_ms is None else round(loop_ms, 3),
            "loop_over_set": None if loop_ms is None else round(loop_ms / max(min(c[0] for c in cmp_ms), 1e-9), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-len", type=int, default=20_000_000)
    ap.add_argument("--mm-genome-len", type=int, default=2_000_000)
    ap.add_argument("--samples", default="2,8,32")
    ap.add_argument("--scaffolds", type=int, default=200)
    ap.add_argument("--distinct", type=int, default=8, help="different synthetic samples made (and resident) per leg")
    ap.add_argument("--loop-max", type=int, default=8, help="run the compare_scaffolds pair loop up to this many samples")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    from instrain_amd import engine
    from tests import util
    ctx = engine.Context(0)
    lut, fb = util.load_lut()
    ctx.set_null_model(lut, fb)
    out = []
    for S in (int(x) for x in args.samples.split(",")):
        out.append(leg(ctx, "one_level", args.genome_len, 3, True, S, args))
        print(json.dumps(out[-1]), flush=True)
        out.append(leg(ctx, "six_levels", args.mm_genome_len, 20, False, S, args))
        print(json.dumps(out[-1]), flush=True)
    ctx.close()
    if args.tag:
        path = os.path.join(REPO, "profiles", "%s_compare_set.md" % args.tag)
        with open(path, "w") as f:
            f.write("# A sample set compared from sketches next to the pair loop (tools/bench_compare_set.py)\n\n")
            f.write("compare_device_ms: event-timed isx_cmpset_compare, all %d repeats; add: wall ms of isx_cmpset_add (the call waits for the "
                    "device); pair_loop_device_ms: the event-timed isx_compare_scaffolds calls of the same pairs on resident batches, summed "
                    "(up to %d samples).  %d different synthetic samples per leg, repeated.\n\n" % (args.reps, args.loop_max, args.distinct))
            keys = list(out[0].keys())
            f.write("| " + " | ".join(keys) + " |\n|" + "---|" * len(keys) + "\n")
            for r in out:
                f.write("| " + " | ".join(str(r[k]) for k in keys) + " |\n")
        print("wrote", path)


if __name__ == "__main__":
    main()
