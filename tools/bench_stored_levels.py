#!/usr/bin/env python3
"""The level passes on a STORED profile (engine.StoredLevels: isx_stored_*, k_level_sparse) next to the same calls on the resident
live batch the profile came from: event-timed device ms, best of --reps, of summarize, genome_coverage and profile_genes, plus the
host time of stored.pack_levels and of the upload (StoredLevels()).

The two shapes of tools/bench_genes.py: skip-mm (--genome-len positions, one level: the live source is the batch's dense tables) and
mm on (--mm-genome-len positions, every level: the live source is the entry table, scanned once per level).  The stored profile is
the batch's own fetched tables cut into per-scaffold series, every split a scaffold; genomes of eight consecutive scaffolds; the gene
set of bench_genes.py.  python tools/bench_stored_levels.py [--tag r07] -> profiles/<tag>_stored_levels.md"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))


def series_of(e, M, bounds, scaffolds):
    """the batch's fetched tables as {scaffold: {mm: (positions, values)}} for covT, clonT, clonTR"""
    covT, clonT, clonTR = {}, {}, {}
    if M == 1:
        cols = [(e["counts"].sum(axis=1).astype(np.int64), covT, lambda a: a > 0), (e["clon"], clonT, lambda a: ~np.isnan(a)),
                (e["clon_r"], clonTR, lambda a: ~np.isnan(a))]
        for j, sc in enumerate(scaffolds):
            a0, a1 = int(bounds[j]), int(bounds[j + 1])
            for arr, dst, keep in cols:
                k = np.flatnonzero(keep(arr[a0:a1]))
                if len(k):
                    dst[sc] = {0: (k, arr[a0:a1][k])}
        return covT, clonT, clonTR
    en = e["entries"]
    cuts = np.searchsorted(en["gpos"], bounds)
    for j, sc in enumerate(scaffolds):
        s = en[cuts[j]:cuts[j + 1]]
        pos, lvl = s["gpos"].astype(np.int64) - int(bounds[j]), s["cnt"].sum(axis=1).astype(np.int64)
        for m in np.unique(s["mm"]):
            at = s["mm"] == m
            covT.setdefault(sc, {})[int(m)] = (pos[at & (lvl > 0)], lvl[at & (lvl > 0)])
            for col, dst in (("clon", clonT), ("clon_rarefied", clonTR)):
                k = at & ~np.isnan(s[col])
                dst.setdefault(sc, {})[int(m)] = (pos[k], s[col][k])
    return covT, clonT, clonTR


def leg(ctx, w, M, args, rng, label):
    from bench_genes import synth_genes
    from instrain_amd import engine
    from instrain_amd.profile import gene_profile, stored
    b = engine.Batch(ctx, w["ref_codes"], w["split_bounds"], w["obs"], w["pair"], n_mm_bins=M, enable_linkage=False)
    b.run()
    bounds = np.asarray(w["split_bounds"], np.int64)            # every split a scaffold
    scaffolds = ["sc%d" % j for j in range(len(bounds) - 1)]
    genome = (np.arange(len(scaffolds)) // 8).astype(np.int32)
    n_genomes = int(genome.max()) + 1
    s2i, s2s = synth_genes(rng, scaffolds, bounds, w["ref_codes"])
    gs = gene_profile.GeneSet(ctx, s2i, s2s)
    gf, gl = gs.call(scaffolds, bounds)
    e = b.fetch()
    covT, clonT, clonTR = series_of(e, M, bounds, scaffolds)
    t0 = time.perf_counter()
    pack = stored.pack_levels(scaffolds, np.diff(bounds), covT, clonT, clonTR, mm_values=list(range(M)))
    pack_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    st = engine.StoredLevels(ctx, pack)
    upload_s = time.perf_counter() - t0
    out = {"leg": label, "n_pos": int(bounds[-1]), "levels": M, "n_scaffolds": len(scaffolds),
           "entries_cov": int(len(pack["cov_gpos"])), "entries_clon": int(len(pack["clon_gpos"])), "entries_clonr": int(len(pack["clonr_gpos"])),
           "live_entries": int(b.sizes()["n_entries"]), "pack_levels_host_s": round(pack_s, 3), "upload_host_s": round(upload_s, 3)}
    differs = []
    for name, live, sto in (("summarize", lambda: b.summarize(bounds), lambda: st.summarize()),
                            ("genome_coverage", lambda: b.genome_coverage(bounds, genome, n_genomes), lambda: st.genome_coverage(bounds, genome, n_genomes)),
                            ("profile_genes", lambda: b.profile_genes(gs.genes, bounds, gf, gl), lambda: st.profile_genes(gs.genes, bounds, gf, gl))):
        lm, sm = [], []
        for _ in range(args.reps):
            rl = live()
            lm.append(rl[-1])
            rs = sto()
            sm.append(rs[-1])
        for k, (x, y) in enumerate(zip(rl[:-1], rs[:-1])):
            for f in (x.dtype.names or [None]):
                if f is not None and name == "summarize" and f.startswith("sum_clon"):
                    continue                        # float sums by atomics in another order
                xa, ya = (x, y) if f is None else (x[f], y[f])
                if xa.tobytes() != ya.tobytes():
                    differs.append("%s output %d%s: %d of %d" % (name, k, "" if f is None else "." + f, int((xa != ya).sum()), xa.size))
        out[name + "_live_ms"], out[name + "_stored_ms"] = round(min(lm), 4), round(min(sm), 4)
    out["stored_equals_live"] = not differs
    if differs:
        out["differs"] = differs
    st.close()
    gs.close()
    b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-len", type=int, default=20_000_000)
    ap.add_argument("--mm-genome-len", type=int, default=2_000_000)
    ap.add_argument("--coverage", type=float, default=3)
    ap.add_argument("--reps", type=int, default=3)
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
        path = os.path.join(REPO, "profiles", "%s_stored_levels.md" % args.tag)
        with open(path, "w") as f:
            f.write("# level passes on a stored profile next to the live batch (tools/bench_stored_levels.py)\n\n")
            f.write("Event-timed device ms, best of %d, of the whole pass (materialisation of every level + the pass's own kernels); "
                    "pack / upload = host seconds of stored.pack_levels and of StoredLevels().  Not measured: the files "
                    "(store_profile / load_profile), the SNV and linkage roll-ups (the same calls on either path), iRep.\n\n" % args.reps)
            keys = list(dict.fromkeys(k for r in out for k in r))
            f.write("| | " + " | ".join(r["leg"] for r in out) + " |\n|---|" + "---|" * len(out) + "\n")
            for k in keys[1:]:
                f.write("| " + k + " | " + " | ".join(str(r.get(k, "")) for r in out) + " |\n")
        print("wrote", path)


if __name__ == "__main__":
    main()
