"""SNV pooling across samples restated in numpy / pandas from observation arrays (test infrastructure; imports nothing of the product).

The rules (inStrain polymorpher.py):
  1. a sample's own rows: its SNV table without the cryptic rows, then the highest-mm row of every (scaffold, position)
  2. a sample has a scaffold when it has a read there; a scaffold is pooled when more than one sample has it
  3. the sites of a pooled scaffold: the union of the own positions of the samples that have it
  4. DSTdb: one row per (sample that has the scaffold, site): the own row's counts where there is one, else the counts of all the
     sample's reads at the position (every mm level), zeros where there is none
  5. PMdb: per site the sums over those rows, the detection counts, the class counts and con_bases of the own rows, ref_base, and the
     con_base / var_base of the sums
The SNV tables come from the oracle (oracle.profile_split) on the same observations.
"""
import numpy as np
import pandas as pd

from oracle import oracle

CH = np.array(list("ACTGN"))
CLASSES = ["AmbiguousReference", "DivergentSite", "SNS", "SNV", "con_SNV", "pop_SNV"]
PM_COLUMNS = ["A", "C", "T", "G", "scaffold", "depth", "ref_base", "sample_5x_detections", "sample_detections", "DivergentSite_count",
              "SNS_count", "SNV_count", "con_SNV_count", "pop_SNV_count", "sample_con_bases", "con_base", "var_base"]


def own_rows(snv):
    """oracle SNV rows of one (sample, scaffold) -> {position: row}: not cryptic, highest mm"""
    out = {}
    for r in snv[np.argsort(snv["mm"], kind="stable")]:
        if not r["cryptic"]:
            out[int(r["pos"])] = r
    return out


def pooled_tables(samples, seq, names, lengths, lut, fallback, min_cov=5, min_freq=0.05):
    """samples: [(name, pos, base, mm)] in insertion order, pos in the flat space of the scaffolds laid end to end, mm = real values.
    -> (DSTdb, PMdb) shaped as compare.SampleSet.pooled_tables() makes them"""
    sb = np.r_[0, np.cumsum(lengths)].astype(np.int64)
    own, reads = {}, {}
    for name, pos, base, mm in samples:
        pos, base, mm = np.asarray(pos, np.int64), np.asarray(base), np.asarray(mm, np.int64)
        for sc in range(len(names)):
            k = (pos >= sb[sc]) & (pos < sb[sc + 1])
            if not k.any():
                continue
            p, b = pos[k] - sb[sc], base[k]
            snv = oracle.profile_split(p, b, mm[k], np.arange(int(k.sum())), seq[sb[sc]:sb[sc + 1]], 0, lut, fallback, min_cov=min_cov,
                                       min_freq=min_freq)["snv"]
            own[(name, sc)] = own_rows(snv)
            table = np.zeros((int(lengths[sc]), 4), np.int64)
            np.add.at(table, (p[b < 4], b[b < 4].astype(np.int64)), 1)
            reads[(name, sc)] = table
    dst, pms, cats = [], [], []
    for sc, scaffold in enumerate(names):
        members = [name for name, *_ in samples if (name, sc) in reads]
        sites = sorted(set().union(*[set(own[(m, sc)]) for m in members])) if len(members) > 1 else []
        if not sites:
            continue
        cats.append(scaffold)
        rows = {}
        for m in members:
            for p in sites:
                r = own[(m, sc)].get(p)
                rows[(m, p)] = np.asarray(r["cnt"], np.int64) if r is not None else reads[(m, sc)][p]
                dst.append((m, p, *rows[(m, p)].tolist(), scaffold))
        for p in sites:
            mine = [own[(m, sc)][p] for m in members if p in own[(m, sc)]]
            tot = sum(rows[(m, p)] for m in members)
            con_bases = list(dict.fromkeys(str(CH[r["con_base"]]) for r in mine))
            rest = tot.copy()
            rest[int(np.argmax(tot))] = 0
            pms.append((p, *tot.tolist(), scaffold, int(tot.sum()), CH[mine[0]["ref_base"]],
                        sum(int(rows[(m, p)].sum() >= 5) for m in members), sum(int(rows[(m, p)].any()) for m in members),
                        *[sum(CLASSES[r["cls"]] == c for r in mine) for c in CLASSES[1:]], str(np.array(con_bases, dtype=object)),
                        CH[int(np.argmax(tot))], CH[rest.tolist().index(rest.max())]))
    cat = pd.CategoricalDtype(cats)
    d = pd.DataFrame(dst, columns=["sample", "position", "A", "C", "T", "G", "scaffold"])
    d = d.set_index(["sample", "position"])
    d.index.names = [None, None]
    d["scaffold"] = d["scaffold"].astype(cat)
    p = pd.DataFrame(pms, columns=["position"] + PM_COLUMNS).set_index("position")
    p.index.name = None
    p["scaffold"] = p["scaffold"].astype(cat)
    for c in ("ref_base", "con_base", "var_base", "sample_con_bases"):
        p[c] = p[c].astype(object)
    return d, p


def load_golden(golden_dir, names):
    """the reference's DSTdb / PMdb as the generator stored them, rows by (scaffold in `names` order, the reference's order inside)"""
    import os
    d = pd.read_csv(os.path.join(golden_dir, "pool_DSTdb.csv"))
    p = pd.read_csv(os.path.join(golden_dir, "pool_PMdb.csv"))
    cat = pd.CategoricalDtype([n for n in names if n in set(d["scaffold"])])
    out = []
    for t, idx in ((d, ["sample", "position"]), (p, ["position"])):
        t["scaffold"] = t["scaffold"].astype(cat)
        t = t.sort_values("scaffold", kind="stable").set_index(idx)
        t.index.names = [None] * len(idx)
        out.append(t)
    return out[0], out[1]


def same_frames(got, exp):
    """two tables: the same index, columns (in order), dtypes and values"""
    assert list(got.columns) == list(exp.columns), (list(got.columns), list(exp.columns))
    assert got.index.equals(exp.index), (got.index, exp.index)
    for c in exp.columns:
        if isinstance(exp[c].dtype, pd.CategoricalDtype):
            assert isinstance(got[c].dtype, pd.CategoricalDtype) and list(got[c].cat.categories) == list(exp[c].cat.categories), c
        else:
            assert got[c].dtype == exp[c].dtype, (c, got[c].dtype, exp[c].dtype)
        assert got[c].astype(object).tolist() == exp[c].astype(object).tolist(), c
