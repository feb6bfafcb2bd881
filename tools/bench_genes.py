#!/usr/bin/env python3
"""The gene pass (`inStrain profile -g`) on a resident batch: device ms of its coverage half, SNV half and count_sites next to the
batch's pileup kernel, the bytes the coverage half reads, and the test restatement's host time on the same input (timed on the
first --restate-genes genes and scaled to all of them).

A prodigal-like synthetic gene set is laid over the batch: one gene per ~1.1 kbp, lengths 300-2100 (multiples of 3), both strands,
about one in eight overlapping its neighbour.  Two batches: skip-mm (--genome-len positions, one level) and mm on (C2-sized,
every level).  python tools/bench_genes.py [--tag r07] [--genome-len N] [--mm-genome-len N]
--tag writes profiles/<tag>_genes.md (kernel times of a rocprofv3 run of its own go in by tools/write_profiles.py-style hand edit)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def synth_genes(rng, scaffolds, bounds, ref_codes):
    letters = np.array(list("ACTG"))                 # the library's base codes 0..3
    comp = {'A': 'T', 'C': 'G', 'G': 'C', 'T': 'A'}
    s2i, s2s = {}, {}
    for j, sc in enumerate(scaffolds):
        a0, a1 = int(bounds[j]), int(bounds[j + 1])
        L = a1 - a0
        rows, seqs, p = [], {}, int(rng.integers(0, 200))
        while True:
            glen = 3 * int(rng.integers(100, 700))
            if p + glen > L:
                break
            d = '1' if rng.random() < 0.5 else '-1'
            name = "%s_%d" % (sc, len(rows) + 1)
            s = ''.join(letters[ref_codes[a0 + p:a0 + p + glen]])
            if d == '-1':
                s = ''.join(comp[c] for c in reversed(s))
            rows.append((name, sc, d, False, p, p + glen - 1))
            seqs[name] = s
            p += glen + int(rng.integers(-60, 400)) if rng.random() < 0.125 else glen + int(rng.integers(20, 400))
            p = max(p, rows[-1][4] + 1)
        if rows:
            s2i[sc] = pd.DataFrame(rows, columns=['gene', 'scaffold', 'direction', 'partial', 'start', 'end'])
            s2s[sc] = seqs
    return s2i, s2s


def leg(ctx, w, M, args, rng, label):
    from instrain_amd import engine
    from instrain_amd.profile import gene_profile
    from tests import gene_ref
    b = engine.Batch(ctx, w["ref_codes"], w["split_bounds"], w["obs"], w["pair"], n_mm_bins=M, enable_linkage=False)
    b.run()
    pileup_ms = b.pileup_ms()
    bounds = np.asarray(w["split_bounds"], np.int64)            # every split a scaffold
    scaffolds = ["sc%d" % j for j in range(len(bounds) - 1)]
    s2i, s2s = synth_genes(rng, scaffolds, bounds, w["ref_codes"])
    gs = gene_profile.GeneSet(ctx, s2i, s2s)
    gf, gl = gs.call(scaffolds, bounds)
    cov_ms = []
    for _ in range(args.reps):
        rows, flags, ms = b.profile_genes(gs.genes, bounds, gf, gl)
        cov_ms.append(ms)
    snv = b.fetch()["snv"]
    snv = snv[np.lexsort((snv["mm"], snv["gpos"]))]
    snv_ms, sites_ms = [], []
    for _ in range(args.reps):
        snv_ms.append(gs.genes.profile_snvs(bounds, gf, gl, snv, M)[2])
        sites_ms.append(gs.genes.sites()[1])
    n_genes = gs.names.size
    gene_pos = int(sum(min(e, bounds[j + 1] - bounds[j] - 1) - s + 1 for j, sc in enumerate(scaffolds) if sc in s2i
                       for s, e in zip(s2i[sc]['start'], s2i[sc]['end'])))
    n_pos = int(bounds[-1])
    # per level: the materialisation (dense: counts 16 B + 2 clonalities read, 12 B written; mm: the entry table once per level),
    # the scaffold emptiness pass (cov + clonality: 8 B a position), the gene intervals (8 B a gene position)
    mat = 32 * n_pos if M == 1 else 32 * int(b.sizes()["n_entries"])
    bytes_read = M * (mat + 8 * n_pos + 8 * gene_pos)
    # the restatement (tests/gene_ref.py) on the first genes, scaled
    k = min(args.restate_genes, n_genes)
    t0 = time.perf_counter()
    done = 0
    e = b.fetch()
    for sc in scaffolds:
        if sc not in s2i or done >= k:
            continue
        j = scaffolds.index(sc)
        a0, a1 = int(bounds[j]), int(bounds[j + 1])
        gdb = s2i[sc]
        if M == 1:
            cov = e["counts"][a0:a1].sum(axis=1).astype(np.int64)
            nz = np.flatnonzero(cov)
            covT = {0: pd.Series(cov[nz], index=nz)}
            cl = e["clon"][a0:a1]
            ok = np.flatnonzero(~np.isnan(cl))
            clonT = {0: pd.Series(cl[ok], index=ok)}
        else:
            en = e["entries"][(e["entries"]["gpos"] >= a0) & (e["entries"]["gpos"] < a1)]
            covT = {int(m): pd.Series(en["cnt"][en["mm"] == m].sum(axis=1).astype(np.int64), index=en["gpos"][en["mm"] == m] - a0)
                    for m in np.unique(en["mm"])}
            clonT = {int(m): pd.Series(en["clon"][(en["mm"] == m) & ~np.isnan(en["clon"])],
                                       index=en["gpos"][(en["mm"] == m) & ~np.isnan(en["clon"])] - a0) for m in np.unique(en["mm"])}
        gene_ref.gene_coverage(gdb, covT)
        gene_ref.gene_clonality(gdb, clonT)
        done += len(gdb)
    restate_s = (time.perf_counter() - t0) * n_genes / max(done, 1)
    gs.close()
    b.close()
    return {"leg": label, "n_pos": n_pos, "levels": M, "n_genes": int(n_genes), "gene_positions": gene_pos, "n_snv_rows": int(len(snv)),
            "pileup_ms": round(pileup_ms, 4), "gene_cov_ms": round(min(cov_ms), 4), "gene_snv_ms": round(min(snv_ms), 4),
            "gene_sites_ms": round(min(sites_ms), 4), "cov_over_pileup": round(min(cov_ms) / max(pileup_ms, 1e-9), 3),
            "bytes_read_cov_half": int(bytes_read), "restatement_host_s_scaled": round(restate_s, 2), "restatement_genes_timed": int(done)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-len", type=int, default=20_000_000)
    ap.add_argument("--mm-genome-len", type=int, default=2_000_000)
    ap.add_argument("--coverage", type=float, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--restate-genes", type=int, default=150)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    from instrain_amd import engine, synth
    from tests import util
    ctx = engine.Context(0)
    lut, fb = util.load_lut()
    ctx.set_null_model(lut, fb)
    rng = np.random.default_rng(5)
    out = []
    w = synth.make_workload(genome_len=args.genome_len, coverage=args.coverage, n_sites=args.genome_len // 1000, seed=3, skip_mm=True)
    out.append(leg(ctx, w, 1, args, rng, "skip_mm"))
    del w
    w = synth.make_workload(genome_len=args.mm_genome_len, coverage=20, n_sites=args.mm_genome_len // 1000, seed=2, skip_mm=False)
    out.append(leg(ctx, w, int(w["n_mm_bins"]), args, rng, "mm_on"))
    ctx.close()
    for r in out:
        print(json.dumps(r))
    if args.tag:
        path = os.path.join(REPO, "profiles", "%s_genes.md" % args.tag)
        with open(path, "w") as f:
            f.write("# gene pass on a resident batch (tools/bench_genes.py)\n\n")
            f.write("Event-timed device ms (best of %d); bytes = what the coverage half reads (estimate from the layout); restatement = "
                    "tests/gene_ref.py on the first genes, scaled to all.\n\n" % args.reps)
            keys = list(out[0].keys())
            f.write("| " + " | ".join(keys) + " |\n|" + "---|" * len(keys) + "\n")
            for r in out:
                f.write("| " + " | ".join(str(r[k]) for k in keys) + " |\n")
        print("wrote", path)


if __name__ == "__main__":
    main()
