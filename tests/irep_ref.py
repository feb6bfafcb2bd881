"""iRep restated in fp64 numpy on integer block sums: what isx_irep_* computes, and the exact value that the reference's FFT windows and
iterative line fit (inStrain/irep_utilities.py:22-81) approximate.  Blocks of 100 positions, integer windows of 50 blocks, an integer
filter on the doubled median, a sort of the integer sums, closed-form least squares on the trimmed points."""
import numpy as np

WINDOW, SLIDE, MASK = 5000, 100, 100
WIN_BLOCKS = WINDOW // SLIDE
FAIL_KEPT, FAIL_COV, FAIL_R2, FAIL_FRAG, EMPTY, NO_FIT = 1, 2, 4, 8, 16, 32
GOLDEN_FLOATS = ("kept_windows", "avg_cov", "r2", "fragMbp", "unfiltered_raw_iRep")


def layout(lengths, genome, n_genomes, mask=MASK):
    """a Python statement of isx_irep_layout -> (per genome dicts, order, offset)"""
    lengths, genome = [int(x) for x in lengths], [int(g) for g in genome]
    gens, order, offset = [], [], [-1] * len(lengths)
    block = window = 0
    for g in range(n_genomes):
        mine = sorted([i for i in range(len(lengths)) if genome[i] == g], key=lambda i: -lengths[i])     # stable: ties in caller order
        L = 0
        for i in mine:
            if lengths[i] >= 2 * mask:
                offset[i] = L
                L += lengths[i] - 2 * mask
        d = dict(L=L, n_blocks=-(-L // SLIDE), n_windows=(L - WINDOW) // SLIDE + 1 if L >= WINDOW else 0, first_block=block,
                 first_window=window, first_scaffold=len(order), num_contigs=len(mine))
        block += d["n_blocks"]
        window += d["n_windows"]
        order += mine
        gens.append(d)
    order += [i for i in range(len(lengths)) if genome[i] < 0]
    return gens, order, offset


def genome_array(per_scaffold, lengths, order, mask=MASK):
    """generate_genome_coverage_array: per_scaffold[i] = int array of scaffold i or None (no reads: zeros), laid end to end in `order`
    without `mask` positions at either end"""
    parts = []
    for i in order:
        ln = int(lengths[i])
        if ln < 2 * mask:
            continue
        a = np.zeros(ln, dtype=np.int64) if per_scaffold[i] is None else np.asarray(per_scaffold[i], dtype=np.int64)
        parts.append(a[mask:ln - mask])
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)


def block_sums(arr):
    arr = np.asarray(arr, dtype=np.int64)
    n = -(-len(arr) // SLIDE)
    pad = np.zeros(n * SLIDE, dtype=np.int64)
    pad[:len(arr)] = arr
    return pad.reshape(n, SLIDE).sum(axis=1).astype(np.uint64)


def window_sums(blocks, L):
    n = (L - WINDOW) // SLIDE + 1 if L >= WINDOW else 0
    c = np.r_[0, np.cumsum(np.asarray(blocks, dtype=np.int64))]
    return c[WIN_BLOCKS:WIN_BLOCKS + n] - c[:n]


def line_fit(X, Y):
    """the least-squares line y = m x + b in the centred two-pass form, and r2 = 1 - var(residual) / var(y)"""
    mx, my = X.mean(), Y.mean()
    dx, dy = X - mx, Y - my
    with np.errstate(divide="ignore", invalid="ignore"):
        m = float((dx * dy).sum() / (dx * dx).sum())
        b = float(my - m * mx)
        res = (m * X + b) - Y
        r2 = float(1 - res.var() / Y.var())
    return m, b, r2


def trimmed_fit(kept_sorted, L, values=False):
    """-> (m, b, r2) of the line through (X_i, Y_i) after trimming int(n * 0.05) points at either end, or None.  Y_i = log2(S_i / WINDOW)
    of the sorted integer sums, or (values=True) log2 of sorted coverage values, anything below 1e-50 taken as 1e-50"""
    n = len(kept_sorted)
    trim = int(n * 0.05)
    if n - 2 * trim < 3:
        return None
    X = ((np.arange(n, dtype=np.float64) * (float(L) / float(n))).astype(np.int64) + 1).astype(np.float64)[trim:n - trim]
    v = np.asarray(kept_sorted, dtype=np.float64)
    Y = (np.log2(np.maximum(v, 1e-50)) if values else np.log2(v / float(WINDOW)))[trim:n - trim]
    return line_fit(X, Y)


def gc_corrected(S, G, kept, L):
    """_iRep_gc_bias (irep_utilities.py:268-294) + the trimmed fit on the corrected coverage: S / G = the windows' integer coverage / G+C
    sums in window order, kept = the filter's mask -> the GC-corrected iRep (unfiltered_iRep), NaN without a line"""
    cov, gc = S[kept].astype(np.float64) / float(WINDOW), G[kept].astype(np.float64) / float(WINDOW)
    n = len(cov)
    if n == 0:
        return float("nan")
    m, b = line_fit(gc, cov)[:2] if n > 2 else (0.0, 0.0)
    err = np.abs(cov - (m * gc + b))
    cutoff = np.sort(err)[::-1][int(n * 0.01)]
    use = ~(err >= cutoff)
    if use.sum() > 2:
        m, b, r2 = line_fit(gc[use], cov[use])
    else:
        m, b, r2 = 0.0, 0.0, 0.0
    corrected = cov if r2 < 0.0 else cov + (cov.mean() - (m * gc + b))
    fit = trimmed_fit(np.sort(corrected), L, values=True)
    return float("nan") if fit is None else float(2.0 ** (fit[0] * L))


def finish(blocks, L, num_contigs, gc_blocks=None):
    """one genome's row from its block sums (and G+C counts) -> dict with the fields of isx_irep_row"""
    blocks = np.asarray(blocks, dtype=np.uint64)
    nan = float("nan")
    out = dict(L=int(L), num_contigs=int(num_contigs), sum_cov=int(blocks.astype(object).sum()) if len(blocks) else 0, n_windows=0, n_kept=0,
               avg_cov=nan, fragMbp=nan, kept_windows=nan, r2=nan, raw_irep=nan, gc_irep=nan, irep=nan, flags=0)
    if L == 0:
        out["flags"] = EMPTY | NO_FIT
        return out
    S_w = window_sums(blocks, L)
    S = np.sort(S_w)
    W = len(S)
    kept = S[:0]
    if W:
        med2 = 2 * int(S[W // 2]) if W & 1 else int(S[W // 2 - 1]) + int(S[W // 2])
        if med2 > 0:
            kept = S[(S > 0) & (16 * S >= med2) & (2 * S <= 8 * med2)]
            if gc_blocks is not None:
                out["gc_irep"] = gc_corrected(S_w, window_sums(gc_blocks, L), (S_w > 0) & (16 * S_w >= med2) & (2 * S_w <= 8 * med2), L)
    out["n_windows"], out["n_kept"] = W, len(kept)
    out["avg_cov"] = out["sum_cov"] / float(L)
    out["fragMbp"] = num_contigs / (float(L) / 1000000)
    out["kept_windows"] = len(kept) / W if W else nan
    flags = 0
    fit = trimmed_fit(kept, L)
    if fit is None:
        flags |= NO_FIT
    else:
        m, _, out["r2"] = fit
        out["raw_irep"] = float(2.0 ** (m * L))
    if out["kept_windows"] < 0.98:
        flags |= FAIL_KEPT
    if out["avg_cov"] < 5:
        flags |= FAIL_COV
    if out["r2"] < 0.9:
        flags |= FAIL_R2
    if out["fragMbp"] > 175:
        flags |= FAIL_FRAG
    out["flags"] = flags
    out["irep"] = nan if flags else out["raw_irep"]
    return out


def accessory(row):
    """the fields the reference's accessory dict names, from a finish() row or an isx_irep_row"""
    return {"kept_windows": float(row["kept_windows"]), "avg_cov": float(row["avg_cov"]), "r2": float(row["r2"]),
            "fragMbp": float(row["fragMbp"]), "unfiltered_raw_iRep": float(row["raw_irep"]), "unfiltered_iRep": float(row["gc_irep"])}


def rel_diff(a, b):
    a, b = float(a), float(b)
    if np.isnan(a) and np.isnan(b):
        return 0.0
    if a == b:
        return 0.0
    return abs(a - b) / max(abs(a), abs(b))


# ---- the golden runs (tests/golden/make_irep_golden.py) ----
def load_golden():
    """-> (inputs, golden): names, lengths, genome (name per scaffold), genomes (names in stb order), gid, bounds, cov [3, n_pos] per
    stored level, seq (codes A C T G, 4 = N); golden: irep_golden.json"""
    import json
    import os
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    z = np.load(os.path.join(here, "irep_inputs.npz"))
    inp = {"names": [str(x) for x in z["names"]], "lengths": z["lengths"].astype(np.int64), "genome": [str(x) for x in z["genome"]],
           "cov": z["cov"].astype(np.int64), "seq": z["seq"].astype(np.uint8)}
    inp["genomes"] = list(dict.fromkeys(inp["genome"]))
    inp["gid"] = np.array([inp["genomes"].index(g) for g in inp["genome"]], dtype=np.int32)
    inp["bounds"] = np.r_[0, np.cumsum(inp["lengths"])].astype(np.int64)
    inp["stb"] = dict(zip(inp["names"], inp["genome"]))
    with open(os.path.join(here, "irep_golden.json")) as f:
        golden = json.load(f)
    return inp, golden


def run_levels(inp, run):
    """a golden run as a device batch sees it -> (cov [n_levels, n_pos] per level, not cumulated; the real mm of every level)"""
    mm_of, use = run["mm_of_level"], run["use_levels"]
    mms = sorted(set(mm_of))
    return np.stack([sum(inp["cov"][lv] for lv, m in zip(use, mm_of) if m == mm) for mm in mms]), mms


def golden_rows(inp, run):
    """finish() of every genome of a golden run from the stored coverage and sequences alone -> list of dicts in inp["genomes"] order"""
    cov, mms = run_levels(inp, run)
    top = [i for i, m in enumerate(mms) if run["skip_mm_profiling"] or m <= 1]
    c = cov[top].sum(axis=0) if top else np.zeros(cov.shape[1], dtype=np.int64)
    gens, order, _ = layout(inp["lengths"], inp["gid"], len(inp["genomes"]))
    per = [c[inp["bounds"][i]:inp["bounds"][i + 1]] for i in range(len(inp["names"]))]
    is_gc = ((inp["seq"] == 1) | (inp["seq"] == 3)).astype(np.int64)
    per_gc = [is_gc[inp["bounds"][i]:inp["bounds"][i + 1]] for i in range(len(inp["names"]))]
    rows = []
    for g, d in enumerate(gens):
        mine = order[d["first_scaffold"]:d["first_scaffold"] + d["num_contigs"]]
        arr = genome_array(per, inp["lengths"], mine)
        assert len(arr) == d["L"]
        rows.append(finish(block_sums(arr), d["L"], d["num_contigs"], block_sums(genome_array(per_gc, inp["lengths"], mine))))
    return rows


def to_struct(rows, dtype):
    out = np.zeros(len(rows), dtype=dtype)
    for i, r in enumerate(rows):
        for k in dtype.names:
            out[k][i] = r.get(k, float("nan"))
    return out
