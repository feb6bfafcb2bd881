#!/usr/bin/env python3
"""The genome_info roll-ups on a resident batch: device ms of isx_batch_genome_coverage (histogram pass, no sort) next to
isx_batch_summarize_genomes (one sort of the position array per level) on the same batch, and of the two row passes
(isx_snv_level_counts, isx_ld_level_sums) on the batch's own rows, next to the batch's pileup kernel.

Every split of the synthetic workload is a scaffold; genomes are --scaffolds-per-genome consecutive scaffolds so that both coverage
calls apply.  Two batches: skip-mm (--genome-len positions, one level) and mm on (--mm-genome-len, every level).
python tools/bench_genomes.py [--tag r08] [--genome-len N] [--mm-genome-len N]
--tag writes profiles/<tag>_genomes.md."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def leg(ctx, w, M, args, label):
    from instrain_amd import engine
    b = engine.Batch(ctx, w["ref_codes"], w["split_bounds"], w["obs"], w["pair"], n_mm_bins=M, enable_linkage=True)
    b.run()
    pileup_ms = b.pileup_ms()
    bounds = np.asarray(w["split_bounds"], np.int64)            # every split a scaffold
    n_scaf = len(bounds) - 1
    first = np.r_[np.arange(0, n_scaf, args.scaffolds_per_genome), n_scaf].astype(np.int32)
    n_gen = len(first) - 1
    sg = (np.arange(n_scaf) // args.scaffolds_per_genome).astype(np.int32)
    sort_ms, hist_ms = [], []
    for _ in range(args.reps):
        lv, ms = b.summarize_genomes(bounds, first, mask_edges=100)
        sort_ms.append(ms)
    for _ in range(args.reps):
        acc, hist, ms = b.genome_coverage(bounds, sg, n_gen, mask_edges=100, hist_bins=args.hist_bins)
        hist_ms.append(ms)
    same = bool((acc["n"] == lv["n"]).all() and (acc["sum_cov"] == lv["sum_cov"]).all() and (acc["sumsq_cov"] == lv["sumsq_cov"]).all())
    res = b.fetch()
    snv, ld = res["snv"], res["ld"]
    snv_ms = [engine.snv_level_counts(ctx, snv, bounds, M)[1] for _ in range(args.reps)]
    ld_ms = [engine.ld_level_sums(ctx, ld, bounds, M)[1] for _ in range(args.reps)]
    n_pos = int(bounds[-1])
    b.close()
    return {"leg": label, "n_pos": n_pos, "levels": M, "n_scaffolds": n_scaf, "n_genomes": n_gen, "hist_bins": int(hist.shape[-1]),
            "max_cov": int(acc["max_cov"].max()), "n_snv_rows": int(len(snv)), "n_ld_rows": int(len(ld)), "pileup_ms": round(pileup_ms, 4),
            "summarize_genomes_ms": [round(x, 4) for x in sort_ms], "genome_coverage_ms": [round(x, 4) for x in hist_ms],
            "sort_over_hist": round(min(sort_ms) / max(min(hist_ms), 1e-9), 2), "same_sums": same,
            "snv_level_counts_ms": round(min(snv_ms), 4), "ld_level_sums_ms": round(min(ld_ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-len", type=int, default=20_000_000)
    ap.add_argument("--mm-genome-len", type=int, default=2_000_000)
    ap.add_argument("--coverage", type=float, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scaffolds-per-genome", type=int, default=35)
    ap.add_argument("--hist-bins", type=int, default=4096)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    from instrain_amd import engine, synth
    from tests import util
    ctx = engine.Context(0)
    lut, fb = util.load_lut()
    ctx.set_null_model(lut, fb)
    out = []
    w = synth.make_workload(genome_len=args.genome_len, coverage=args.coverage, n_sites=args.genome_len // 1000, seed=3, skip_mm=True)
    out.append(leg(ctx, w, 1, args, "skip_mm"))
    del w
    w = synth.make_workload(genome_len=args.mm_genome_len, coverage=20, n_sites=args.mm_genome_len // 1000, seed=2, skip_mm=False)
    out.append(leg(ctx, w, int(w["n_mm_bins"]), args, "mm_on"))
    ctx.close()
    for r in out:
        print(json.dumps(r))
    if args.tag:
        path = os.path.join(REPO, "profiles", "%s_genomes.md" % args.tag)
        with open(path, "w") as f:
            f.write("# genome_info roll-ups on a resident batch (tools/bench_genomes.py)\n\n")
            f.write("Event-timed device ms; the two coverage calls list all %d repeats (the spread), the row passes the best of them.  "
                    "summarize_genomes = the sort per level (isx_batch_summarize_genomes); genome_coverage = the histogram pass "
                    "(isx_batch_genome_coverage) on the same batch, genomes of %d consecutive scaffolds.\n\n" % (args.reps, args.scaffolds_per_genome))
            keys = list(out[0].keys())
            f.write("| " + " | ".join(keys) + " |\n|" + "---|" * len(keys) + "\n")
            for r in out:
                f.write("| " + " | ".join(str(r[k]) for k in keys) + " |\n")
        print("wrote", path)


if __name__ == "__main__":
    main()
