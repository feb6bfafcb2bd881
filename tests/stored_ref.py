"""Stored-profile inputs for the compare tests, made by numpy / pandas alone (never imports the product): a sample's covT as
`inStrain compare` loads it from raw_data/covT.hd5 ({scaffold: {mm: pd.Series(coverage, index=positions)}}) and its
cumulative_snv_table in the reference's columns."""
import numpy as np
import pandas as pd

BASES = np.array(["A", "C", "T", "G", "N"])
SNV_COLUMNS = ["scaffold", "position", "position_coverage", "allele_count", "ref_base", "con_base", "var_base", "A", "C", "T", "G", "mm"]


def covT_from_obs(pos, base, real_mm, bounds, names):
    """observations (flat position, base code 0..3 = A C T G / 4 = N, real mm) over the scaffolds [bounds[i], bounds[i + 1]) ->
    {scaffold: {mm: Series}}: per level the count of A/C/T/G observations of every position that has one.  A key exists iff it has
    an entry; a scaffold without any is not in the dict."""
    pos, base, real_mm = np.asarray(pos, dtype=np.int64), np.asarray(base), np.asarray(real_mm, dtype=np.int64)
    out = {}
    for sc, name in enumerate(names):
        k = (base < 4) & (pos >= bounds[sc]) & (pos < bounds[sc + 1])
        d = {}
        for m in np.unique(real_mm[k]).tolist():
            p, n = np.unique(pos[k & (real_mm == m)] - bounds[sc], return_counts=True)
            d[int(m)] = pd.Series(n.astype("int32"), index=p.astype("int"))
        if d:
            out[name] = d
    return out


def load_stored_golden(path):
    """tests/golden/stored_compare_inputs.npz -> (scaffold names, lengths, sample names, {sample: covT}, {sample: SNV table})"""
    z = np.load(path)
    names, lengths, samples = [str(n) for n in z["names"]], [int(n) for n in z["lengths"]], [str(s) for s in z["samples"]]
    covT, tables = {}, {}
    for s in samples:
        off, d = z[s + "_cov_off"], {}
        for k, (sc, mm) in enumerate(zip(z[s + "_cov_scaffold"].tolist(), z[s + "_cov_mm"].tolist())):
            d.setdefault(names[sc], {})[mm] = pd.Series(z[s + "_cov_val"][off[k]:off[k + 1]].astype("int32"),
                                                        index=z[s + "_cov_pos"][off[k]:off[k + 1]].astype("int"))
        covT[s] = d
        cols = [c for c in SNV_COLUMNS if s + "_snv_" + c in z.files]
        tables[s] = pd.DataFrame({c: z[s + "_snv_" + c].astype(object if z[s + "_snv_" + c].dtype.kind == "U" else np.int64) for c in cols})
    return names, lengths, samples, covT, tables


def snv_frame(rows, bounds, names, mm_values=None):
    """SNV rows (fields gpos in the flat space, mm = level, con_base / ref_base / var_base codes, allele_count, cnt[4] = A C T G) ->
    the cumulative_snv_table: the reference's columns, bases as letters, mm = mm_values[level] (None: the level itself)"""
    rows = np.asarray(rows)
    if len(rows) == 0:
        return pd.DataFrame()
    bounds = np.asarray(bounds, dtype=np.int64)
    g = rows["gpos"].astype(np.int64)
    sc = np.searchsorted(bounds, g, side="right") - 1
    cnt = rows["cnt"].astype(np.int64)
    mm = rows["mm"].astype(np.int64)
    if mm_values is not None:
        mm = np.asarray(mm_values, dtype=np.int64)[mm]
    db = pd.DataFrame({"scaffold": np.asarray(names, dtype=object)[sc], "position": g - bounds[sc], "position_coverage": cnt.sum(axis=1),
                       "allele_count": rows["allele_count"].astype(np.int64), "ref_base": BASES[np.minimum(rows["ref_base"], 4)],
                       "con_base": BASES[rows["con_base"]], "var_base": BASES[rows["var_base"]],
                       "A": cnt[:, 0], "C": cnt[:, 1], "T": cnt[:, 2], "G": cnt[:, 3], "mm": mm}, columns=SNV_COLUMNS)
    return db
