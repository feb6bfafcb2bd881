"""Plain numpy, float64 restatement of the per-scaffold summary (isx_summary.hip run_summary) and of the coverage half of the per-pair
compare (run_compare), written from the observations and never from device output.  tests/test_summary_ref.py pins it against
oracle/summary.py, oracle/compare.py and the stored golden tables; tests/test_gpu_summary_edges.py and tests/test_gpu_compare_edges.py
hold the kernels against it.

Levels: `cov_levels[m]` is the cumulative coverage of every position up to level m (np.bincount of the ACGT observations with mm <= m,
what tests/test_gpu_rollup_edges.py::_cov_levels does).  `clon_levels[m]` is, per position, the clonality of the highest level <= m that
has one (get_basewise_clons), NaN where there is none.  They come from oracle.profile_split scaffold by scaffold (oracle_levels), or --
for large inputs -- vectorised from the cumulative base counts (clon_levels_from_counts; the host test shows the two agree bit for bit).
The rarefied clonalities are random in the reference, so nothing independent can state them: entry_levels() lays out the product's own
per-(position, mm) values the same way, and the summary of THOSE is what the device's rarefied columns are held against."""
import math

import numpy as np

TILE = 64                       # positions per lane of k_seg_reduce / k_overlap_reduce
BLOCK = 256 * TILE              # positions per workgroup
BIG_SEG = 1 << 17               # run_summary: longer segments go to the device-wide radix sort
FIELDS = ("nonzero", "sum_cov", "sumsq_cov", "median_cov", "counted", "sum_clon", "median_clon", "counted_rarefied", "sum_clon_rarefied",
          "median_clon_rarefied", "present")


def cov_levels(gpos, base, mm, n_pos, M):
    """[M, n_pos] int64: cumulative coverage per level; a non-ACGT observation (base > 3) counts nothing"""
    gpos, base, mm = np.asarray(gpos, dtype=np.int64), np.asarray(base), np.asarray(mm)
    k = base < 4
    return np.stack([np.bincount(gpos[k & (mm <= j)], minlength=n_pos) for j in range(M)]).astype(np.int64)


def presence(gpos, base, mm, bounds, M):
    """[n_scaffolds, M] bool: the covT keys of every scaffold.  Several levels (the entries path): a level is there as soon as one
    observation of that level lies on the scaffold, a non-ACGT one included (update_covT stores a 0, shrink_basewise keeps the key).
    One level (the dense path): the scaffold has coverage."""
    gpos, base, mm = np.asarray(gpos, dtype=np.int64), np.asarray(base), np.asarray(mm, dtype=np.int64)
    bounds = np.asarray(bounds, dtype=np.int64)
    sc = np.searchsorted(bounds, gpos, side="right") - 1
    out = np.zeros((len(bounds) - 1, M), dtype=bool)
    if M == 1:
        out[sc[base < 4], 0] = True
    else:
        out[sc, mm] = True
    return out


def clonality(counts):
    """calculate_clonality (snv_utilities.py:225-231) of [n, 4] counts with a non-zero sum: float64 in source order (the sum of the four
    squared frequencies, left to right), stored as float32 like clonT -> float64 array of float32 values"""
    c = np.asarray(counts, dtype=np.float64)
    s = c.sum(axis=1)
    f = c / s[:, None]
    prob = f[:, 0] * f[:, 0]
    for k in (1, 2, 3):
        prob = prob + f[:, k] * f[:, k]
    return prob.astype(np.float32).astype(np.float64)


def clon_levels_from_counts(gpos, base, mm, n_pos, M, min_cov=5):
    """[M, n_pos] float64: level m's value is the clonality of the counts up to m where they reach min_cov.  (A level without an entry
    at a position leaves its counts, hence the value of the level below, unchanged: the carry-over of get_basewise_clons.)"""
    gpos, base, mm = np.asarray(gpos, dtype=np.int64), np.asarray(base, dtype=np.int64), np.asarray(mm)
    out = np.full((M, n_pos), np.nan)
    for j in range(M):
        k = (base < 4) & (mm <= j)
        cnt = np.bincount(gpos[k] * 4 + base[k], minlength=4 * n_pos).reshape(n_pos, 4)
        ok = cnt.sum(axis=1) >= min_cov
        out[j, ok] = clonality(cnt[ok])
    return out


def entry_levels(pos, mm, values, n_pos, M):
    """per-(position, mm) values (NaN = none) -> [M, n_pos] float64: at level m the value of the highest level <= m that has one"""
    pos, mm, values = np.asarray(pos, dtype=np.int64), np.asarray(mm, dtype=np.int64), np.asarray(values, dtype=np.float64)
    out = np.full((M, n_pos), np.nan)
    for j in range(M):
        if j:
            out[j] = out[j - 1]
        k = (mm == j) & ~np.isnan(values)
        out[j, pos[k]] = values[k]
    return out


def oracle_levels(bounds, gpos, base, mm, pair, seq, M, lut, fb, min_cov=5, min_freq=0.05):
    """oracle.profile_split on every scaffold's own observations (CPU, independent of the device)
    -> (clon_levels [M, n_pos], list of the per-scaffold results with scaffold-relative positions)"""
    from oracle import oracle
    gpos = np.asarray(gpos, dtype=np.int64)
    n_pos = int(bounds[-1])
    clon = np.full((M, n_pos), np.nan)
    results = []
    for s0, s1 in zip(bounds[:-1], bounds[1:]):
        s0, s1 = int(s0), int(s1)
        k = (gpos >= s0) & (gpos < s1)
        r = oracle.profile_split(gpos[k] - s0, np.asarray(base)[k], np.asarray(mm)[k], np.asarray(pair)[k], seq[s0:s1], 0, lut, fb,
                                 min_cov=min_cov, min_freq=min_freq)
        e = r["entries"]
        clon[:, s0:s1] = entry_levels(e["pos"], e["mm"], e["clon"], s1 - s0, M)
        results.append(r)
    return clon, results


def _median(x):
    x = x[~np.isnan(x)]
    return float(np.median(x)) if len(x) else float("nan")


def scaffold_levels(cov_levels, clon_levels, clon_r_levels, present, bounds):
    """-> {field: [n_scaffolds, M] array} with the fields of isx_scaffold_level: nonzero, sum_cov, sumsq_cov (int64, exact),
    median_cov (np.median), counted / sum_clon (math.fsum) / median_clon over the non-NaN clonalities (the median NaN when there are
    none) and the same three of the rarefied ones, present"""
    M, n_seg = len(cov_levels), len(bounds) - 1
    out = {f: np.zeros((n_seg, M), dtype=np.int64 if f in ("nonzero", "sum_cov", "sumsq_cov", "counted", "counted_rarefied") else
                       bool if f == "present" else np.float64) for f in FIELDS}
    out["present"][:] = np.asarray(present, dtype=bool)
    for i, (s0, s1) in enumerate(zip(bounds[:-1], bounds[1:])):
        for m in range(M):
            c = np.asarray(cov_levels[m][int(s0):int(s1)], dtype=np.int64)
            assert c.max(initial=0) < 2 ** 31                   # c * c below stays inside int64 for any scaffold of the uint32 flat space
            out["nonzero"][i, m], out["sum_cov"][i, m], out["sumsq_cov"][i, m] = np.count_nonzero(c), c.sum(), (c * c).sum()
            out["median_cov"][i, m] = np.median(c)
            for lev, cnt, sm, med in ((clon_levels, "counted", "sum_clon", "median_clon"),
                                      (clon_r_levels, "counted_rarefied", "sum_clon_rarefied", "median_clon_rarefied")):
                v = np.asarray(lev[m][int(s0):int(s1)], dtype=np.float64)
                v = v[~np.isnan(v)]
                out[cnt][i, m], out[sm][i, m], out[med][i, m] = len(v), math.fsum(v), _median(v)
    return out


def sum_bound(n, exact):
    """how far a float64 sum of n non-negative terms, added in ANY order (atomics), may lie from math.fsum of them: recursive summation
    loses at most (n - 1) * 2**-53 * sum|x| (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2, to first order),
    plus one ulp of the result for fsum's own rounding"""
    return max(int(n) - 1, 0) * 2.0 ** -53 * abs(exact) + float(np.spacing(abs(exact)))


def pair_levels(cov_a_levels, cov_b_levels, present_a, present_b, bounds, min_cov):
    """calc_mm2overlap per scaffold -> {both, either, present_a, present_b: [n_scaffolds, max(M_a, M_b)]}.  A sample's coverage carries
    over beyond its own last level, where it has no key of its own (present 0)."""
    Ma, Mb = len(cov_a_levels), len(cov_b_levels)
    M, n_seg = max(Ma, Mb), len(bounds) - 1
    out = {"both": np.zeros((n_seg, M), dtype=np.int64), "either": np.zeros((n_seg, M), dtype=np.int64),
           "present_a": np.zeros((n_seg, M), dtype=bool), "present_b": np.zeros((n_seg, M), dtype=bool)}
    out["present_a"][:, :Ma] = np.asarray(present_a, dtype=bool)
    out["present_b"][:, :Mb] = np.asarray(present_b, dtype=bool)
    for m in range(M):
        a = np.asarray(cov_a_levels[min(m, Ma - 1)]) >= min_cov
        b = np.asarray(cov_b_levels[min(m, Mb - 1)]) >= min_cov
        for i, (s0, s1) in enumerate(zip(bounds[:-1], bounds[1:])):
            out["both"][i, m] = int((a & b)[int(s0):int(s1)].sum())
            out["either"][i, m] = int((a | b)[int(s0):int(s1)].sum())
    return out


def overlap_dicts(pl):
    """pair_levels' arrays as compare.calc_mm2overlap returns them: per scaffold {mm: both} and {mm: both / either (0 when nothing is
    covered)} over the union of the two samples' keys"""
    o, c = [], []
    for i in range(len(pl["both"])):
        keys = np.flatnonzero(pl["present_a"][i] | pl["present_b"][i])
        o.append({int(m): int(pl["both"][i, m]) for m in keys})
        c.append({int(m): (pl["both"][i, m] / pl["either"][i, m] if pl["either"][i, m] > 0 else 0) for m in keys})
    return o, c
