#!/usr/bin/env python3
"""A sample entering a comparison set from its STORED profile (compare.SampleSet.add_profile, isx_cmpset_add_profile) next to the same
sample entering from its resident batch (add_batch), on two synthetic samples: --genome-len positions with one level, --mm-genome-len
positions with 6 levels (--scaffolds scaffolds each).  Per leg, --reps times each into a fresh set:
  add_batch_wall_ms   isx_cmpset_add of the resident batch -- wall ms, the call waits for the device (the yardstick)
  pack_ms             compare.pack_profile: covT Series + SNV table -> the arrays of the C call (host, numpy)
  h2d_ms              a plain pageable host-to-device copy of the same positions / values arrays (hipMemcpy), for scale
  call_wall_ms        isx_cmpset_add_profile as a whole: host checks, upload, device pass, wait
  device_ms           its event-timed device pass (k_profile_planes + the SNV tail)
  device_GBps         (8 B per coverage entry read + the plane words written) / device_ms
python tools/bench_compare_stored.py [--tag r13]      --tag writes profiles/<tag>_compare_stored.md."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def stored_profile(batch, sb, names):
    """the batch's tables as a stored profile: covT {scaffold: {mm: Series}} and the cumulative_snv_table"""
    import pandas as pd
    r = batch.fetch()
    if "counts" in r:
        cov = r["counts"].sum(axis=1, dtype=np.int64)
        gpos, mm = np.flatnonzero(cov), None
        cov = cov[gpos]
    else:
        e = r["entries"]
        cov = e["cnt"].sum(axis=1, dtype=np.int64)
        keep = cov > 0
        gpos, mm, cov = e["gpos"][keep].astype(np.int64), e["mm"][keep].astype(np.int64), cov[keep]
    covT = {}
    sc = np.searchsorted(sb, gpos, side="right") - 1
    for lv in ([0] if mm is None else np.unique(mm).tolist()):
        k = slice(None) if mm is None else mm == lv
        g, s, c = gpos[k], sc[k], cov[k]
        order = np.lexsort((g, s))
        g, s, c = g[order], s[order], c[order]
        cut = np.searchsorted(s, np.arange(len(names) + 1))
        for i, n in enumerate(names):
            if cut[i + 1] > cut[i]:
                covT.setdefault(n, {})[int(lv)] = pd.Series(c[cut[i]:cut[i + 1]].astype("int32"), index=(g[cut[i]:cut[i + 1]] - sb[i]).astype("int"))
    v = r["snv"]
    vs = np.searchsorted(sb, v["gpos"].astype(np.int64), side="right") - 1
    bases = np.array(list("ACTGN"))
    cnt = v["cnt"].astype(np.int64)
    table = pd.DataFrame({"scaffold": np.array(names, dtype=object)[vs], "position": v["gpos"].astype(np.int64) - sb[vs], "mm": v["mm"].astype(np.int64),
                          "con_base": bases[v["con_base"]], "ref_base": bases[np.minimum(v["ref_base"], 4)], "var_base": bases[v["var_base"]],
                          "allele_count": v["allele_count"].astype(np.int64), "A": cnt[:, 0], "C": cnt[:, 1], "T": cnt[:, 2], "G": cnt[:, 3]})
    return covT, table


_hip = None


def plain_upload_ms(arrays):
    """wall ms of one synchronous hipMemcpy per array, pageable host memory -> a fresh device buffer (allocation not timed); None when
    the HIP runtime cannot be loaded by name: not measured"""
    global _hip
    import ctypes as C
    import ctypes.util
    if _hip is None:
        for cand in (ctypes.util.find_library("amdhip64"), "libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
            try:
                _hip = C.CDLL(cand) if cand else None
            except OSError:
                _hip = None
            if _hip is not None:
                break
        if _hip is None:
            _hip = False
    if not _hip:
        return None
    total = 0.0
    for a in arrays:
        ptr = C.c_void_p()
        if a.nbytes == 0:
            continue
        if _hip.hipMalloc(C.byref(ptr), C.c_size_t(a.nbytes)) != 0:
            return None
        t0 = time.perf_counter()
        _hip.hipMemcpy(ptr, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1)          # hipMemcpyHostToDevice
        total += (time.perf_counter() - t0) * 1e3
        _hip.hipFree(ptr)
    return total


def leg(ctx, label, genome_len, coverage, skip_mm, args):
    from instrain_amd import compare, engine, synth
    lens = [genome_len // args.scaffolds] * args.scaffolds
    lens[-1] += genome_len - sum(lens)
    sb = np.r_[0, np.cumsum(lens)].astype(np.int64)
    names = ["s%d" % i for i in range(args.scaffolds)]
    w = synth.make_workload(genome_len=genome_len, coverage=coverage, n_sites=genome_len // 1000, seed=11, skip_mm=skip_mm, max_mm=5)
    b = engine.Batch(ctx, w["ref_codes"], w["split_bounds"], w["obs"], w["pair"], n_mm_bins=int(w["n_mm_bins"]), enable_linkage=False)
    b.run()
    del w
    covT, table = stored_profile(b, sb, names)
    mm_values = list(range(b.n_mm_bins))
    batch_ms, pack_ms, h2d_ms, call_ms, dev_ms = [], [], [], [], []
    same = None
    for _ in range(args.reps):
        live = compare.SampleSet(ctx, names, lens, min_cov=5)
        t0 = time.perf_counter()
        live.add_batch("x", b, names, sb)
        batch_ms.append((time.perf_counter() - t0) * 1e3)
        st = compare.SampleSet(ctx, names, lens, min_cov=5)
        t0 = time.perf_counter()
        p = compare.pack_profile(st.index, st.lengths, covT, table, mm_values)
        pack_ms.append((time.perf_counter() - t0) * 1e3)
        h2d_ms.append(plain_upload_ms([p["positions"], p["values"]]))
        t0 = time.perf_counter()
        st.add_packed("x", p)
        call_ms.append((time.perf_counter() - t0) * 1e3)
        dev_ms.append(st.profile_device_ms)
        if same is None:                                        # the two routes leave the same sketch: each against itself and the other
            for s in (live, st):
                s.add_batch("y", b, names, sb)
                s.compare()
            same = live.levels.tobytes() == st.levels.tobytes()
        live.close()
        st.close()
    b.close()
    n_entries, L = len(p["positions"]), len(p["levels"])
    plane_bytes = L * 8 * int(sum((ln + 63) // 64 for ln in lens))
    r2 = lambda xs: [None if x is None else round(float(x), 3) for x in xs]
    return {"leg": label, "n_pos": int(genome_len), "levels": L, "scaffolds": args.scaffolds, "entries": n_entries, "snv_rows": len(p["snv"]),
            "same_sketch_as_add_batch": same, "add_batch_wall_ms": r2(batch_ms), "pack_ms": r2(pack_ms), "h2d_ms": r2(h2d_ms),
            "call_wall_ms": r2(call_ms), "device_ms": r2(dev_ms), "device_MB": round((8 * n_entries + plane_bytes) / 1e6, 2),
            "device_GBps": round((8 * n_entries + plane_bytes) / 1e6 / max(min(dev_ms), 1e-9), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-len", type=int, default=20_000_000)
    ap.add_argument("--mm-genome-len", type=int, default=2_000_000)
    ap.add_argument("--scaffolds", type=int, default=200)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    from instrain_amd import engine
    from tests import util
    ctx = engine.Context(0)
    lut, fb = util.load_lut()
    ctx.set_null_model(lut, fb)
    out = []
    for label, n, cov, skip in (("one_level", args.genome_len, 3, True), ("six_levels", args.mm_genome_len, 20, False)):
        out.append(leg(ctx, label, n, cov, skip, args))
        print(json.dumps(out[-1]), flush=True)
    ctx.close()
    if args.tag:
        path = os.path.join(REPO, "profiles", "%s_compare_stored.md" % args.tag)
        with open(path, "w") as f:
            f.write("# A sample into a comparison set from its stored profile, next to add_batch (tools/bench_compare_stored.py)\n\n")
            f.write("All %d repeats of every figure, each into a fresh set (the first repeat also pays first-use set-up).  add_batch_wall_ms: "
                    "isx_cmpset_add of the resident batch, wall (the call waits); pack_ms: compare.pack_profile on the host; h2d_ms: a plain "
                    "pageable copy of the same positions / values arrays, for scale; call_wall_ms: isx_cmpset_add_profile as a whole (host "
                    "checks, upload, device pass, wait); device_ms: its event-timed device pass; device_GBps: (8 B per entry + the plane words "
                    "written) over the fastest device_ms.\n\n" % args.reps)
            keys = list(out[0].keys())
            f.write("| " + " | ".join(keys) + " |\n|" + "---|" * len(keys) + "\n")
            for r in out:
                f.write("| " + " | ".join(str(r[k]) for k in keys) + " |\n")
        print("wrote", path)


if __name__ == "__main__":
    main()
