#!/usr/bin/env python3
"""tests/golden/make_irep_golden.py -- golden vectors of iRep at the genome level.

Runs ONLY in the build container (needs the reference checkout): imports the reference's own inStrain.genomeUtilities and
inStrain.irep_utilities under the stub importer of make_golden.py and calls
  genomeLevel_coverage_info (genomeUtilities.py:297-365) on a duck-typed covT with a scaff2sequence of lists
      -> the iRep / iRep_GC_corrected columns of every run
  generate_genome_coverage_array (:932-981) + calculate_iRep_from_coverage_array (irep_utilities.py:22-81)
      -> the accessory dict of every genome
on synthetic genomes: Poisson coverage whose mean falls by a factor of two from the middle of a genome to either end, split over the mm
levels 0, 1 and 3.  Only data is stored: irep_inputs.npz (per-scaffold coverage as small integers, sequences as codes, the stb) and
irep_golden.json.

REAL lmfit IS NOT PINNED.  lmfit is not installed here; a stand-in goes into sys.modules before the reference is imported: Parameters and
minimize(method='leastsq') on scipy.optimize.leastsq with lmfit's default tolerances (ftol = xtol = 1.5e-8, gtol = 0,
maxfev = 2000 * (n + 1)).  The value both solvers approximate is the least-squares line; tests/irep_ref.py computes it in closed form, and
`measured_band` records how far the reference's result lies from it on this data.

usage: python tests/golden/make_irep_golden.py
"""
import json
import os
import sys
import types
import warnings

import numpy as np
import pandas as pd
import scipy.optimize

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


# ---- the lmfit stand-in ----
class _Par:
    def __init__(self, value):
        self.value = value


class _Parameters(dict):
    def add(self, name, value=None, vary=True):
        self[name] = _Par(value)


class _Result:
    pass


def _minimize(fcn, params, args=(), kws=None, method="leastsq"):
    assert method == "leastsq"
    names = list(params)

    def f(x):
        for n, v in zip(names, x):
            params[n].value = float(v)
        return np.asarray(fcn(params, *args, **(kws or {})), dtype=np.float64)

    x0 = [float(params[n].value) for n in names]
    x = scipy.optimize.leastsq(f, x0, ftol=1.5e-8, xtol=1.5e-8, gtol=0.0, maxfev=2000 * (len(x0) + 1))[0]
    r = _Result()
    r.residual = f(x)
    r.params = params
    return r


_lm = types.ModuleType("lmfit")
_lm.Parameters, _lm.minimize = _Parameters, _minimize
sys.modules["lmfit"] = _lm

import make_golden as mg                                        # noqa: E402  (the stub importer)

mg.import_reference()
import inStrain.genomeUtilities as gu                           # noqa: E402
import inStrain.irep_utilities as iu                            # noqa: E402
from tests import irep_ref                                      # noqa: E402

assert iu.lmfit is _lm
rng = np.random.Generator(np.random.PCG64(1909))
LEVELS = [0, 1, 3]
SHARE = [0.8, 0.15, 0.05]               # of the coverage, per level


def profile(L, depth):
    """mean coverage over a genome of L positions: depth in the middle, half of it at either end"""
    x = np.arange(L, dtype=np.float64)
    return depth * 2.0 ** (-np.abs(x - L / 2) / (L / 2))


# genome -> (scaffold lengths, mean coverage over the concatenated UNMASKED array or None = no reads at all, per scaffold covered?)
def genome_pass():
    return [9103, 6151, 5337], lambda L: profile(L, 16.0), None


def genome_r2():
    def mean(L):                         # two plateaus a factor of five apart, the higher one short: nothing a line fits
        m = np.full(L, 8.0)
        m[3 * L // 4:] = 40.0
        return m
    return [12060, 8045], mean, None


def genome_kept():
    def mean(L):                         # a stretch of 9 000 positions at the end, more than 8 x under the median: ~45 windows fall wholly
        m = profile(L, 12.0)             # into it and are dropped; the ~44 that straddle its edge are kept, and the trim (5 % of ~900)
        m[L - 9000:] = 0.2               # takes them off the fit, so r2 stays high
        return m
    return [98250], mean, None


def genome_cov():
    return [14222, 7411], lambda L: profile(L, 4.0), None


def genome_frag():
    lens = [150, 199, 200, 201] + list(range(470, 526))
    return lens, lambda L: profile(L, 16.0), None


def genome_short():
    return [3000], lambda L: profile(L, 12.0), None


def genome_empty():
    return [140, 180], lambda L: profile(L, 12.0), None


def genome_noreads():
    return [21033, 1500], lambda L: profile(L, 16.0), [True, False]       # the second scaffold has a length but no reads


def genome_even():
    return [17300], lambda L: profile(L, 12.0), None                     # L 17 100: 122 windows


def genome_odd():
    return [17400], lambda L: profile(L, 12.0), None                     # L 17 200: 123 windows


GENOMES = {"pass": genome_pass, "r2": genome_r2, "kept": genome_kept, "cov": genome_cov, "frag": genome_frag, "short": genome_short,
           "empty": genome_empty, "noreads": genome_noreads, "even": genome_even, "odd": genome_odd}

names, lengths, stb, cov_levels, seqs = [], [], {}, [], []
for g, make in GENOMES.items():
    lens, mean, covered = make()
    # the mean is laid over the masked, concatenated array in the reference's order (longest first); the masked edges get the edge value
    order = sorted(range(len(lens)), key=lambda i: -lens[i])
    Lm = sum(max(ln - 200, 0) for ln in lens if ln >= 200)
    m = mean(Lm) if Lm else np.zeros(0)
    at, per = 0, {}
    for i in order:
        ln = lens[i]
        full = np.zeros(ln)
        if ln >= 200:
            full[100:ln - 100] = m[at:at + ln - 200]
            full[:100], full[ln - 100:] = full[100], full[ln - 101]
            at += ln - 200
        else:
            full[:] = 10.0
        if covered is not None and not covered[i]:
            full[:] = 0.0
        per[i] = full
    for i, ln in enumerate(lens):
        sc = "%s_s%02d" % (g, i)
        names.append(sc)
        lengths.append(ln)
        stb[sc] = g
        cov_levels.append(np.stack([rng.poisson(per[i] * s) for s in SHARE]).astype(np.uint8))
        seqs.append(rng.choice(5, ln, p=[0.27, 0.22, 0.27, 0.22, 0.02]).astype(np.uint8))   # codes A C T G, 4 = N
assert len(set(lengths)) == len(lengths), "distinct lengths: the reference's order among equal ones is unspecified"
cov_all = np.concatenate(cov_levels, axis=1)
assert cov_all.max() < 255
bounds = np.r_[0, np.cumsum(lengths)]
s2l = dict(zip(names, lengths))
CH = "ACTGN"
scaff2sequence = {sc: [CH[c] for c in seqs[i]] for i, sc in enumerate(names)}
bin2scaffolds = {}
for sc, g in stb.items():
    bin2scaffolds.setdefault(g, set()).add(sc)

# run -> (the stored levels it uses, the mm value of each, the table's mms, skip_mm_profiling)
RUNS = {"mm013": ([0, 1, 2], [0, 1, 3], None, False), "mm02": ([0, 1], [0, 2], None, False), "skip": ([0, 1, 2], [0, 0, 0], [1000], True)}


def make_covT(use, mm_of):
    covT = {}
    for i, sc in enumerate(names):
        per_mm = {}
        for lv, mm in zip(use, mm_of):
            per_mm[mm] = per_mm.get(mm, 0) + cov_levels[i][lv].astype(np.int64)
        covT[sc] = {}
        for mm, c in per_mm.items():
            nz = np.flatnonzero(c)
            if len(nz):
                covT[sc][mm] = pd.Series(c[nz].astype("int32"), index=nz.astype(np.int64))
        if not covT[sc]:
            del covT[sc]                # no reads at all: not a key of covT
    return covT


golden = {"runs": {}, "genomes": list(GENOMES), "levels": LEVELS}
band, band_detail = 0.0, {}
for run, (use, mm_of, mms, skip) in RUNS.items():
    covT = make_covT(use, mm_of)
    mms = sorted(set(mm_of)) if mms is None else mms
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = gu.genomeLevel_coverage_info(covT, bin2scaffolds, set(GENOMES), s2l, scaff2sequence, mms)
    rows = []
    for _, r in ref.iterrows():
        fl = r["iRep_GC_corrected"]
        rows.append({"genome": r["genome"], "mm": int(r["mm"]), "iRep": None if pd.isna(r["iRep"]) else float(r["iRep"]),
                     "iRep_GC_corrected": None if (not isinstance(fl, (bool, np.bool_)) and pd.isna(fl)) else bool(fl)})
    entry = {"mm_of_level": mm_of, "use_levels": use, "mms": mms, "skip_mm_profiling": skip, "table": rows, "accessory": {}}
    max_mm = 1000 if skip else 1
    if skip or 1 in mms:
        for g in GENOMES:
            scaffolds = sorted(bin2scaffolds[g], key=s2l.get, reverse=True)
            covs, _ = gu.generate_genome_coverage_array(covT, s2l, order=scaffolds, maxMM=max_mm, mask_edges=100)
            L = len(covs)
            gens, order, _ = irep_ref.layout([s2l[s] for s in scaffolds], [0] * len(scaffolds), 1)
            assert gens[0]["L"] == L
            gc_arr = np.concatenate([np.isin(scaff2sequence[s][100:s2l[s] - 100], ["G", "C"]).astype(np.int64) for s in scaffolds
                                     if s2l[s] >= 200] or [np.zeros(0, dtype=np.int64)])
            mine = irep_ref.finish(irep_ref.block_sums(np.asarray(covs, dtype=np.int64)), L, len(scaffolds), irep_ref.block_sums(gc_arr))
            acc = {"L": L, "num_contigs": len(scaffolds), "n_windows": mine["n_windows"], "n_kept": mine["n_kept"], "sum_cov": mine["sum_cov"],
                   "flags": mine["flags"]}
            if L >= irep_ref.WINDOW:       # below, the reference's 'valid' convolution swaps its operands: other windows, NaN either way
                gcw = iu.generate_gc_windows(scaffolds, scaff2sequence, mask_edges=100)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    val, junk = iu.calculate_iRep_from_coverage_array(covs, len(scaffolds), gcw)
                assert junk["iRep_GC_corrected"] is True
                acc["iRep"] = None if np.isnan(val) else float(val)
                assert (mine["irep"] != mine["irep"]) == (acc["iRep"] is None), (run, g, mine, junk)
                for k in irep_ref.GOLDEN_FLOATS + ("unfiltered_iRep",):
                    acc[k] = float(junk[k])
                    d = irep_ref.rel_diff(junk[k], irep_ref.accessory(mine)[k])
                    band_detail["%s/%s/%s" % (run, g, k)] = d
                    band = max(band, d)
                # no value within 1e-3 relative of its threshold
                for k, thr in (("r2", 0.9), ("avg_cov", 5.0), ("kept_windows", 0.98), ("fragMbp", 175.0)):
                    assert abs(float(junk[k]) - thr) > 1e-3 * thr, (run, g, k, junk[k])
            entry["accessory"][g] = acc
    golden["runs"][run] = entry
golden["measured_band"] = band
golden["band_detail"] = band_detail

acc = golden["runs"]["mm013"]["accessory"]
want = {"pass": 0, "r2": irep_ref.FAIL_R2, "kept": irep_ref.FAIL_KEPT, "cov": irep_ref.FAIL_COV, "frag": irep_ref.FAIL_FRAG}
for g, f in want.items():
    assert acc[g]["flags"] == f, (g, acc[g])
assert acc["empty"]["L"] == 0 and 0 < acc["short"]["L"] < 5000
assert acc["even"]["n_windows"] % 2 == 0 and acc["odd"]["n_windows"] % 2 == 1
assert all(r["iRep"] is None and r["iRep_GC_corrected"] is None for r in golden["runs"]["mm02"]["table"])

with open(os.path.join(HERE, "irep_golden.json"), "w") as f:
    json.dump(golden, f, indent=1, sort_keys=True)
np.savez_compressed(os.path.join(HERE, "irep_inputs.npz"), names=np.array(names), lengths=np.array(lengths, dtype=np.int64),
                    genome=np.array([stb[s] for s in names]), cov=cov_all, seq=np.concatenate(seqs), levels=np.array(LEVELS))
for run, e in golden["runs"].items():
    print(run, [(r["genome"], r["mm"], r["iRep"], r["iRep_GC_corrected"]) for r in e["table"]][:12])
    for g, a in e["accessory"].items():
        print("   ", g, a)
print("measured_band", band)
