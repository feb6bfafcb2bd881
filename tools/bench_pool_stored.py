#!/usr/bin/env python3
"""Pooling from stored profiles and observations (SampleSet.add_profile_pooled / pool_add_obs) next to the live route (add_batch /
pool_add) on the workloads of tools/bench_pool.py, and k_pull_obs with wave aggregation next to the plain-atomics build.

legs      the synthetic --genome-len one-level sample and the --mm-genome-len six-level sample of tools/bench_pool.py, --samples samples
          (--distinct different workloads over one reference, repeated), 50 scaffolds.  For the SAME sample, wall ms of the call (it waits
          for the device):  add_batch | add_profile_pooled (the packed profile: pack_profile's host time is given apart) with its
          event-timed device ms;  pool_add | pool_add_obs (every observation of the sample, one region per scaffold, one call) with its
          event-timed kernel ms.  The two sets' count and meta columns are checked equal.
kernel    one scaffold, every --site-every-th position a site another sample owns, --obs observations column by column at depths 10
          and 500 in ONE pool_add_obs call; the two builds (the in-tree library; `make -C instrain_amd/csrc pull_plain`, through ISX_LIB)
          run in child processes of their own, alternating --rounds times.
Every figure is the best (and the median) of --reps calls after one warm-up call, each on fresh state (a fresh set for the adds, a fresh
pool_sites() for the pulls).
python tools/bench_pool_stored.py [--tag T]        --tag writes profiles/<T>_pool_stored.md."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PLAIN = os.path.join(REPO, "instrain_amd", "libinstrain_amd_pull_plain.so")
CLASSES = np.array(["AmbiguousReference", "DivergentSite", "SNS", "SNV", "con_SNV", "pop_SNV"], dtype=object)


def _stat(v):
    v = np.asarray(v[1:], dtype=np.float64)                    # (the first call is the warm-up)
    return round(float(v.min()), 4), round(float(np.median(v)), 4)


def _covT(obs, sb, names, n_levels):
    """{scaffold: {mm: (positions, values)}} of a workload's observations: one bincount over (level, position)"""
    n = int(sb[-1])
    k = obs["base"] < 4
    cnt = np.bincount(obs["mm"][k].astype(np.int64) * n + obs["gpos"][k].astype(np.int64), minlength=n * n_levels).reshape(n_levels, n)
    out = {}
    for sc, name in enumerate(names):
        d = {}
        for mm in range(n_levels):
            c = cnt[mm, sb[sc]:sb[sc + 1]]
            p = np.flatnonzero(c)
            if len(p):
                d[mm] = (p, c[p])
        if d:
            out[name] = d
    return out


def leg(ctx, label, genome_len, coverage, skip_mm, args):
    from instrain_amd import compare, engine, synth
    from tests import stored_ref
    S = args.samples
    lens = [genome_len // args.scaffolds] * args.scaffolds
    lens[-1] += genome_len - sum(lens)
    sb = np.r_[0, np.cumsum(lens)].astype(np.int64)
    names = ["s%d" % i for i in range(args.scaffolds)]
    batches, works, packed, pack_ms, regions = [], [], [], [], []
    index = {n: i for i, n in enumerate(names)}
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
        rows = b.fetch()["snv"]
        table = stored_ref.snv_frame(rows, sb, names)
        table["class"], table["cryptic"] = CLASSES[rows["cls"]], rows["cryptic"].astype(bool)
        covT = _covT(w["obs"], sb, names, int(w["n_mm_bins"]))
        t0 = time.perf_counter()
        packed.append(compare.pack_profile(index, lens, covT, table, mm_values=list(range(int(w["n_mm_bins"]))), pool=True))
        pack_ms.append((time.perf_counter() - t0) * 1e3)
        order = np.argsort(w["obs"]["gpos"], kind="stable")
        obs = np.ascontiguousarray(w["obs"][order])
        regions.append((obs, np.searchsorted(obs["gpos"], sb).astype(np.int64)))
    add_batch, add_prof, add_prof_dev = [], [], []
    A = B = None
    for rep in range(args.reps + 1):                            # fresh sets: an add is timed on a sample the set does not have yet
        for st in (A, B):
            if st is not None:
                st.close()
        A = compare.SampleSet(ctx, names, lens, min_cov=5, pooling=True)
        B = compare.SampleSet(ctx, names, lens, min_cov=5, pooling=True)
        ta, tb, td = [], [], []
        for k in range(S):
            t0 = time.perf_counter()
            A.add_batch("sample%d" % k, batches[k % len(batches)], names, sb)
            ta.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            B._add_packed("sample%d" % k, packed[k % len(packed)], 1 << 26, True)
            tb.append((time.perf_counter() - t0) * 1e3)
            td.append(B.profile_device_ms)
        add_batch.append(np.median(ta)); add_prof.append(np.median(tb)); add_prof_dev.append(np.median(td))
    pull_batch, pull_obs, pull_obs_dev = [], [], []
    n_obs = int(np.median([len(r[0]) for r in regions]))
    for rep in range(args.reps + 1):
        n_sites = A.pool_sites()
        assert B.pool_sites() == n_sites
        ta, tb, td = [], [], []
        for k in range(S):
            t0 = time.perf_counter()
            A.pool_add("sample%d" % k, batches[k % len(batches)], names, sb)
            ta.append((time.perf_counter() - t0) * 1e3)
            obs, off = regions[k % len(regions)]
            t0 = time.perf_counter()
            ms = B.pool_add_obs("sample%d" % k, names, obs, off, gpos0=sb[:-1])
            tb.append((time.perf_counter() - t0) * 1e3)
            td.append(ms)
            B.pool_obs_done("sample%d" % k, names)
        pull_batch.append(np.median(ta)); pull_obs.append(np.median(tb)); pull_obs_dev.append(np.median(td))
    A.pooled_tables()
    B.pooled_tables()
    same = all(A.pool_raw[f].tobytes() == B.pool_raw[f].tobytes() for f in ("summary", "counts", "meta"))
    assert same, "the stored route's bytes differ from the live route's"
    A.close()
    B.close()
    for b in batches:
        b.close()
    r = {"leg": label, "n_pos": int(genome_len), "samples": S, "sites": int(n_sites), "obs_per_sample": n_obs,
         "pack_profile_host_ms": round(float(np.median(pack_ms)), 1)}
    for key, v in (("add_batch_wall_ms", add_batch), ("add_profile_pooled_wall_ms", add_prof), ("add_profile_pooled_device_ms", add_prof_dev),
                   ("pool_add_wall_ms", pull_batch), ("pool_add_obs_wall_ms", pull_obs), ("pool_add_obs_kernel_ms", pull_obs_dev)):
        r[key + "_best"], r[key + "_median"] = _stat(v)
    return r


def kernel_ab(args):
    import pandas as pd
    from instrain_amd import _lib, compare, engine
    ctx = engine.Context(0)
    rng = np.random.Generator(np.random.PCG64(9))
    out = []
    for depth in (10, 500):
        n_pos = max(args.obs // depth, 64)
        sites = np.arange(0, n_pos, args.site_every)
        st = compare.SampleSet(ctx, ["g"], [n_pos], min_cov=5, pooling=True)
        cov = {"g": {0: (np.arange(n_pos), np.full(n_pos, 10))}}
        table = pd.DataFrame({"scaffold": "g", "position": sites, "mm": 0, "con_base": "A", "ref_base": "A", "var_base": "C", "allele_count": 2,
                              "A": 5, "C": 5, "T": 0, "G": 0, "class": "SNV", "cryptic": False})
        st.add_profile_pooled("owner", cov, table)
        st.add_profile_pooled("puller", cov, pd.DataFrame())
        obs = engine.pack_obs(np.repeat(np.arange(n_pos, dtype=np.uint32), depth), rng.integers(0, 4, n_pos * depth).astype(np.uint8),
                              np.zeros(n_pos * depth, np.int64))
        dev = []
        for rep in range(args.reps + 1):
            st.pool_sites()
            dev.append(st.pool_add_obs("puller", ["g"], obs, [0, len(obs)]))
        c, meta = np.zeros((len(sites), 4), np.uint32), np.zeros(len(sites), np.uint8)
        _lib.check(st.lib.isx_cmpset_pool_fetch_sample(st.h, 1, c.ctypes.data, meta.ctypes.data))
        assert int(c.sum()) == len(sites) * depth, (int(c.sum()), len(sites) * depth)       # every observation at a site counted once
        st.close()
        best, med = _stat(dev)
        out.append({"depth": depth, "sites": int(len(sites)), "observations": int(len(obs)), "kernel_ms_best": best, "kernel_ms_median": med})
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-len", type=int, default=2_000_000)
    ap.add_argument("--mm-genome-len", type=int, default=500_000)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--scaffolds", type=int, default=50)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--obs", type=int, default=64_000_000, help="observations of the kernel A/B (512 MB: more than the last-level cache)")
    ap.add_argument("--site-every", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--tag", default="")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(kernel_ab(args)), flush=True)
        return
    if not os.path.exists(PLAIN):
        raise SystemExit("%s not built: make -C instrain_amd/csrc pull_plain" % PLAIN)
    # the kernel A/B first, in child processes, while this process has not touched the device yet
    ab = []
    for rnd in range(args.rounds):
        for label, env in (("plain atomics", dict(os.environ, ISX_LIB=PLAIN)), ("wave runs", dict(os.environ))):
            env.pop("ISX_LIB", None) if label == "wave runs" else None
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--obs", str(args.obs), "--site-every", str(args.site_every),
                                  "--reps", str(args.reps)], env=env, capture_output=True, text=True, timeout=600)
            line = [x for x in res.stdout.splitlines() if x.startswith("RESULT ")]
            if res.returncode or not line:
                raise SystemExit("the %s child failed:\n" % label + res.stdout[-2000:] + res.stderr[-2000:])
            for r in json.loads(line[0][7:]):
                ab.append(dict(r, kernel=label, round=rnd))
                print(json.dumps(ab[-1]), flush=True)
    from instrain_amd import engine
    from tests import util
    ctx = engine.Context(0)
    lut, fb = util.load_lut()
    ctx.set_null_model(lut, fb)
    legs = [leg(ctx, "one_level", args.genome_len, 12, True, args)]
    print(json.dumps(legs[-1]), flush=True)
    legs.append(leg(ctx, "six_levels", args.mm_genome_len, 20, False, args))
    print(json.dumps(legs[-1]), flush=True)
    ctx.close()
    if args.tag:
        path = os.path.join(REPO, "profiles", "%s_pool_stored.md" % args.tag)
        with open(path, "w") as f:
            f.write("# Pooling from stored profiles and observations next to the live route; k_pull_obs A/B (tools/bench_pool_stored.py)\n\n")
            f.write("Legs: the synthetic samples of tools/bench_pool.py, %d samples (%d different workloads over one reference, repeated), %d "
                    "scaffolds.  Wall ms of the call, which waits for the device; per figure best / median over %d repetitions after a warm-up "
                    "one, each the median over the samples, on fresh state (fresh sets for the adds, a fresh pool_sites() for the pulls).  "
                    "add_profile_pooled is timed on the packed profile (pack_profile_host_ms apart); pool_add_obs takes every observation of "
                    "the sample in one call from pageable memory (host sweep, upload, kernel, wait); *_device_ms / *_kernel_ms are event-timed.  "
                    "The two sets' summary, count and meta bytes were equal in this run.  The timed windows are single calls of the "
                    "length shown.\n\n" % (args.samples, args.distinct, args.scaffolds, args.reps))
            keys = list(legs[0].keys())
            f.write("| " + " | ".join(keys) + " |\n|" + "---|" * len(keys) + "\n")
            for r in legs:
                f.write("| " + " | ".join(str(r[k]) for k in keys) + " |\n")
            f.write("\nKernel A/B: one scaffold, every %dth position a site another sample owns, every column at the given depth in ONE "
                    "pool_add_obs call (%d observations, %d MB of records: more than the last-level cache holds).  Event-timed kernel ms, best / "
                    "median of %d calls after a warm-up, each after a fresh pool_sites(); the two builds in processes of their own, "
                    "alternating, %d rounds.  The timed window is ONE kernel of the length shown.\n\n"
                    % (args.site_every, args.obs, args.obs * 8 // 1_000_000, args.reps, args.rounds))
            keys = ["kernel", "round", "depth", "sites", "observations", "kernel_ms_best", "kernel_ms_median"]
            f.write("| " + " | ".join(keys) + " |\n|" + "---|" * len(keys) + "\n")
            for r in sorted(ab, key=lambda r: (r["depth"], r["kernel"], r["round"])):
                f.write("| " + " | ".join(str(r[k]) for k in keys) + " |\n")
        print("wrote", path)


if __name__ == "__main__":
    main()
