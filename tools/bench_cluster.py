#!/usr/bin/env python3
"""Strain clustering per genome (compare.linkage_flat / cluster_genome_strains, SampleSet.strain_clusters; isx_cluster.hip), event-timed
device ms of both entry points for --genomes synthetic genomes x S samples (S in --samples):
  table   isx_cluster_linkage: every genome's condensed matrix from the host (a few strains per genome: zeros inside a strain, 1e-3 .. 1e-2
          between strains, some pairs at 1.0) -- all genomes in one call; wall ms of the call with its copies next to it
  set     isx_cmpset_cluster on a set of S samples over --genomes one-scaffold genomes after one isx_cmpset_compare: the failed-scaffold
          pass, the (genome, pair) roll-up and the clustering together (S up to --set-max)
  scipy   the loop the reference runs: scipy.cluster.hierarchy.linkage + fcluster per genome over the same matrices, on the host, wall ms
          (only when scipy imports; the reference's pandas work around it -- iterrows, add_av_RC, the pivot -- is not in this number)
python tools/bench_cluster.py [--tag r12]        --tag writes profiles/<tag>_cluster.md."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def synthetic_matrices(n_genomes, S, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    iu = np.triu_indices(S, 1)
    out = np.zeros((n_genomes, len(iu[0])))
    for g in range(n_genomes):
        strain = rng.integers(0, max(2, S // 4), size=S)
        between = rng.uniform(1e-3, 1e-2, size=(strain.max() + 1,) * 2)
        between = (between + between.T) / 2
        d = np.where(strain[iu[0]] == strain[iu[1]], 0.0, between[strain[iu[0]], strain[iu[1]]])
        d[rng.random(len(d)) < 0.02] = 1.0                      # pairs below the coverage threshold
        out[g] = d
    return out


def table_leg(ctx, S, args):
    from instrain_amd import compare
    mats = synthetic_matrices(args.genomes, S, 100 + S)
    n_points = np.full(args.genomes, S, dtype=np.int32)
    offsets = np.arange(args.genomes, dtype=np.int64) * mats.shape[1]
    row = {"leg": "table", "genomes": args.genomes, "samples": S}
    for method in ("average", "complete", "weighted"):
        dev, wall = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            labels, Z, ms = compare._linkage_batch(ctx, n_points, offsets, mats.ravel(), method, 1e-5)
            wall.append(round((time.perf_counter() - t0) * 1e3, 2))
            dev.append(round(ms, 3))
        row[method + "_device_ms"], row[method + "_wall_ms"] = dev, wall
    try:
        import scipy.cluster.hierarchy as sch
        t0 = time.perf_counter()
        same = True
        ref = [sch.fcluster(sch.linkage(m, method="average"), 1e-5, criterion="distance") for m in mats]
        row["scipy_loop_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        labels, _, _ = compare._linkage_batch(ctx, n_points, offsets, mats.ravel(), "average", 1e-5)
        same = bool((np.concatenate(ref) == labels).all())
        row["labels_equal_scipy"] = same
    except ImportError:
        row["scipy_loop_wall_ms"], row["labels_equal_scipy"] = None, None
    return row


def set_leg(ctx, S, args):
    from instrain_amd import _lib, compare, engine, synth
    G, ln = args.genomes, args.scaffold_len
    lens = [ln] * G
    sb = np.arange(G + 1, dtype=np.int64) * ln
    names = ["g%04d_1" % i for i in range(G)]
    stb = {n: n[:-2] for n in names}
    batches = []
    for k in range(min(S, args.distinct)):
        w = synth.make_workload(genome_len=G * ln, coverage=12, n_sites=G * ln // 500, seed=31 + k, skip_mm=True, max_mm=5)
        b = engine.Batch(ctx, w["ref_codes"], w["split_bounds"], w["obs"], w["pair"], n_mm_bins=int(w["n_mm_bins"]), enable_linkage=False)
        b.run()
        batches.append(b)
        del w
    st = compare.SampleSet(ctx, names, lens, min_cov=5)
    for k in range(S):
        st.add_batch("sample%03d" % k, batches[k % len(batches)], names, sb)
    for b in batches:
        b.close()
    # the comparison itself through the library call alone: SampleSet.compare()'s row dicts are not what is measured here
    n_s, n_a = C.c_int32(0), C.c_int32(0)
    _lib.check(st.lib.isx_cmpset_axis(st.h, C.byref(n_s), C.byref(n_a), None))
    out = np.zeros((S * (S - 1) // 2, G, n_a.value), dtype=_lib.COMPARE_LEVEL_DT)
    ms = C.c_float(0)
    _lib.check(st.lib.isx_cmpset_compare(st.h, 0.05, out.size, out.ctypes.data, C.byref(ms)))
    row = {"leg": "set", "genomes": G, "samples": S, "scaffold_len": ln, "compare_device_ms": round(ms.value, 3)}
    del out
    for method in ("average",):
        dev, wall = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            cdb = st.strain_clusters(stb, clusterAlg=method)
            wall.append(round((time.perf_counter() - t0) * 1e3, 2))
            dev.append(round(st.cluster_device_ms, 3))
        row[method + "_device_ms"], row[method + "_wall_ms"] = dev, wall
    row["clustered"] = int((st.cluster_status["status"] == _lib.CLUSTER_OK).sum())
    row["cdb_rows"], row["clusters"] = len(cdb), int(cdb["cluster"].nunique())
    st.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=1000)
    ap.add_argument("--samples", default="8,32,128")
    ap.add_argument("--set-max", type=int, default=128, help="run the set form up to this many samples")
    ap.add_argument("--scaffold-len", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=8, help="different synthetic samples made per set leg, repeated")
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
        out.append(table_leg(ctx, S, args))
        print(json.dumps(out[-1]), flush=True)
        if S <= args.set_max:
            out.append(set_leg(ctx, S, args))
            print(json.dumps(out[-1]), flush=True)
    ctx.close()
    if args.tag:
        path = os.path.join(REPO, "profiles", "%s_cluster.md" % args.tag)
        with open(path, "w") as f:
            f.write("# Strain clustering per genome on the device next to the scipy loop (tools/bench_cluster.py)\n\n")
            f.write("*_device_ms: event-timed kernels of the call, all %d repeats (the first one includes the first launch of its kernels); "
                    "*_wall_ms: the Python call with its copies and tables; scipy_loop_wall_ms: linkage + fcluster per genome on the host, "
                    "method average, without the reference's pandas work around it.  One run, no other process on the device checked for.\n\n"
                    % args.reps)
            for r in out:
                f.write("- " + json.dumps(r) + "\n")
        print("wrote", path)


if __name__ == "__main__":
    main()
