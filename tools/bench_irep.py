#!/usr/bin/env python3
"""iRep on the device: event-timed device ms of engine.IRep.add (isx_irep_add: one level materialised + the block pass) next to
isx_batch_genome_coverage (one level materialised + the histogram pass) on the same resident skip-mm batch of --genome-len positions,
and of engine.IRep.finish for --finish-genomes genomes whose block sums are loaded through add_blocks.

Every split of the synthetic workload is a scaffold; genomes are --scaffolds-per-genome consecutive scaffolds.
python tools/bench_irep.py [--tag r10] [--genome-len N]
--tag writes profiles/<tag>_irep.md."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def add_leg(ctx, args):
    from instrain_amd import engine, synth
    w = synth.make_workload(genome_len=args.genome_len, coverage=args.coverage, n_sites=args.genome_len // 1000, seed=3, skip_mm=True)
    b = engine.Batch(ctx, w["ref_codes"], w["split_bounds"], w["obs"], w["pair"], n_mm_bins=1, enable_linkage=False)
    b.run()
    bounds = np.asarray(w["split_bounds"], np.int64)
    n_scaf = len(bounds) - 1
    sg = (np.arange(n_scaf) // args.scaffolds_per_genome).astype(np.int32)
    n_gen = int(sg.max()) + 1
    hist_ms = [b.genome_coverage(bounds, sg, n_gen, mask_edges=100)[2] for _ in range(args.reps)]
    add_ms, gc_ms = [], []
    idx = np.arange(n_scaf, dtype=np.int32)
    for _ in range(args.reps):
        ir = engine.IRep(ctx, np.diff(bounds), sg, n_gen)
        add_ms.append(ir.add(b, bounds, idx, 0))
        cov = ir.blocks()[0]
        ir.close()
        ir = engine.IRep(ctx, np.diff(bounds), sg, n_gen)
        gc_ms.append(ir.add(b, bounds, idx, -1))
        ir.close()
    n_pos = int(bounds[-1])
    b.close()
    return {"leg": "add", "n_pos": n_pos, "n_scaffolds": n_scaf, "n_genomes": n_gen, "n_blocks": int(len(cov)),
            "genome_coverage_ms": [round(x, 4) for x in hist_ms], "irep_add_ms": [round(x, 4) for x in add_ms],
            "irep_add_gc_only_ms": [round(x, 4) for x in gc_ms], "add_over_genome_coverage": round(min(add_ms) / max(min(hist_ms), 1e-9), 2)}


def finish_leg(ctx, args):
    from instrain_amd import engine
    rng = np.random.Generator(np.random.PCG64(11))
    lengths = rng.integers(1_000_000, 5_000_000, args.finish_genomes)
    ir = engine.IRep(ctx, lengths, np.arange(len(lengths), dtype=np.int32), len(lengths))
    blocks = rng.poisson(1200, ir.n_blocks).astype(np.uint64)
    ir.add_blocks(blocks)
    ms = [ir.finish()[1] for _ in range(args.reps)]
    rows = ir.finish()[0]
    ir.close()
    return {"leg": "finish", "n_genomes": len(lengths), "n_blocks": int(len(blocks)), "n_windows": int(rows["n_windows"].sum()),
            "finish_ms": [round(x, 4) for x in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-len", type=int, default=20_000_000)
    ap.add_argument("--coverage", type=float, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scaffolds-per-genome", type=int, default=35)
    ap.add_argument("--finish-genomes", type=int, default=1000)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    from instrain_amd import engine
    from tests import util
    ctx = engine.Context(0)
    lut, fb = util.load_lut()
    ctx.set_null_model(lut, fb)
    out = [add_leg(ctx, args), finish_leg(ctx, args)]
    ctx.close()
    for r in out:
        print(json.dumps(r))
    if args.tag:
        path = os.path.join(REPO, "profiles", "%s_irep.md" % args.tag)
        with open(path, "w") as f:
            f.write("# iRep on the device (tools/bench_irep.py)\n\n")
            f.write("Event-timed device ms, all %d repeats of each call (the spread).  irep_add = isx_irep_add at level 0 (one level "
                    "materialised, then the block pass over the coverage array and the reference) next to genome_coverage = "
                    "isx_batch_genome_coverage (one level materialised, then the histogram pass) on the same resident skip-mm batch, genomes "
                    "of %d consecutive scaffolds; irep_add_gc_only = level -1 (the reference alone).  finish = isx_irep_finish (window sums, "
                    "segmented sort, one workgroup per genome for median, kept range and line) on block sums loaded through "
                    "isx_irep_blocks_add.\n\n" % (args.reps, args.scaffolds_per_genome))
            for r in out:
                keys = list(r.keys())
                f.write("| " + " | ".join(keys) + " |\n|" + "---|" * len(keys) + "\n")
                f.write("| " + " | ".join(str(r[k]) for k in keys) + " |\n\n")
        print("wrote", path)


if __name__ == "__main__":
    main()
