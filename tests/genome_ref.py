"""Test-only restatement of the reference's genome-level rules (inStrain v1.9.1 genomeUtilities.py), pandas group by pandas group:
genomeLevel_from_IS (:145-269) = _genomeLevel_scaffold_info_v3 (:545-605) + genomeLevel_coverage_info (:297-365, without iRep) on
generate_genome_coverage_array (:932-981) + _genome_wide_linkage (:636-659), and the merges between them.  The checker of
profile/genome_utilities.py GenomeTables; product code never imports it.  Also: the per-scaffold device rows GenomeTables is fed
with, derived in numpy from stored tables (rows_from_tables)."""
import os

import numpy as np
import pandas as pd

from instrain_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SUM_COLUMNS = ['SNS_count', 'SNV_count', 'divergent_site_count', 'consensus_divergent_sites', 'population_divergent_sites']
NOT_COMPARED = ['iRep', 'iRep_GC_corrected']


def estimate_breadth(coverage):
    return (-1) * np.exp(-1 * ((0.883) * coverage)) + 1


def bin2length(stb, s2l):
    b2l = {}
    for scaffold, genome in stb.items():
        b2l.setdefault(genome, 0)
        if scaffold in s2l:
            b2l[genome] += s2l[scaffold]
    return b2l


def masked_coverage(covT, s2l, scaffolds, mm, mask_edges=100):
    """the coverage of `scaffolds` laid end to end, cumulated over levels <= mm, `mask_edges` positions cut from both ends of each
    (a scaffold shorter than twice that drops out); covT: scaffold -> {mm: Series(position -> coverage)}"""
    arrs = []
    for sc in scaffolds:
        ln = int(s2l[sc])
        cov = np.zeros(ln, dtype=np.float64)
        for m, ser in covT.get(sc, {}).items():
            if int(m) <= int(mm):
                np.add.at(cov, np.asarray(ser.index, dtype=np.int64), np.asarray(ser.values, dtype=np.float64))
        arrs.append(cov[mask_edges:ln - mask_edges] if ln >= 2 * mask_edges else cov[:0])
    return np.concatenate(arrs) if arrs else np.zeros(0)


def scaffold_half(gdb, stb, b2l):
    rows = []
    for mm in sorted(gdb['mm'].unique()):
        odb = gdb[gdb['mm'] <= mm].sort_values('mm').drop_duplicates(subset=['scaffold'], keep='last')
        for genome, df in odb.groupby('genome'):
            r = {'mm': mm, 'genome': genome, 'detected_scaffolds': len(df), 'true_scaffolds': sum(1 for b in stb.values() if b == genome),
                 'length': int(b2l[genome])}
            for col in SUM_COLUMNS:
                r[col] = df[col].fillna(0).sum()
            for col in ('breadth', 'coverage'):
                r[col] = float((df[col].fillna(0) * df['length']).sum()) / b2l[genome]
            considered = df['breadth_minCov'] * df['length']
            total = float(considered.sum())
            for col in ('nucl_diversity', 'nucl_diversity_rarefied'):
                r[col] = float((df[col].fillna(0) * considered).sum()) / total if total != 0 else np.nan
            r['conANI_reference'] = (total - df['consensus_divergent_sites'].sum()) / total if total != 0 else 0
            r['popANI_reference'] = (total - df['population_divergent_sites'].sum()) / total if total != 0 else 0
            r['breadth_minCov'] = total / b2l[genome]
            r['breadth_expected'] = estimate_breadth(r['coverage'])
            rows.append(r)
    return pd.DataFrame(rows)


def calc_snps(sdb, mm):
    """the reference's calc_snps (profile/snv_utilities.py:249-272) on one scaffold's SNV table (columns position, mm, allele_count,
    class): of the rows at levels <= mm every position keeps its highest one -> (SNS, SNV, divergent, consensus, population)"""
    if len(sdb) == 0:
        return 0, 0, 0, 0, 0
    db = sdb[sdb['mm'] <= mm].sort_values('mm').drop_duplicates(subset=['position'], keep='last')
    return (len(db[db['allele_count'] == 1]), len(db[db['allele_count'] > 1]), len(db),
            len(db[db['class'].isin(['SNS', 'con_SNV', 'pop_SNV'])]), len(db[db['class'].isin(['SNS', 'pop_SNV'])]))


def coverage_half(covT, stb, s2l, relevant, mms, mask_edges=100):
    rows = []
    genome2scaffolds = {}
    for sc, g in stb.items():
        genome2scaffolds.setdefault(g, []).append(sc)
    for genome, scaffolds in genome2scaffolds.items():
        if genome not in relevant:
            continue
        for mm in mms:
            covs = masked_coverage(covT, s2l, [s for s in scaffolds if s in s2l], mm, mask_edges)
            if len(covs) == 0:
                covs = np.zeros(1)
            n = len(covs)
            rows.append({'mm': mm, 'genome': genome, 'coverage_median': int(np.median(covs)),
                         'coverage_SEM': float(np.std(covs, ddof=1) / np.sqrt(n)) if n > 1 else np.nan, 'coverage_std': float(np.std(covs))})
    db = pd.DataFrame(rows)
    db['iRep'] = np.nan
    db['iRep_GC_corrected'] = np.nan
    return db


def linkage_half(ldb, mms):
    rows = []
    for mm in mms:
        odb = ldb[ldb['mm'] <= mm].sort_values('mm').drop_duplicates(subset=['scaffold', 'position_A', 'position_B'], keep='last')
        for genome, df in odb.groupby('genome'):
            rows.append({'genome': genome, 'mm': mm, 'r2_mean': df['r2'].mean(), 'd_prime_mean': df['d_prime'].mean(),
                         'SNV_distance_mean': df['distance'].mean(), 'linked_SNV_count': len(df)})
    return pd.DataFrame(rows, columns=['genome', 'mm', 'r2_mean', 'd_prime_mean', 'SNV_distance_mean', 'linked_SNV_count'])


def genome_info(sdb, ldb, covT, stb, s2l, skip_mm_profiling=False, mask_edges=100):
    """sdb: the concatenated cumulative_scaffold_table; ldb: the concatenated raw_linkage_table (may be empty); covT: scaffold ->
    {mm: Series}; -> the table of genomeLevel_from_IS without its reads_* columns"""
    b2l = bin2length(stb, s2l)
    gdb = sdb.copy()
    gdb['scaffold'] = gdb['scaffold'].astype(str)
    gdb['genome'] = gdb['scaffold'].map(stb)
    if skip_mm_profiling:
        gdb = gdb.sort_values('mm').drop_duplicates(subset=['scaffold'], keep='last').sort_values('scaffold')
        gdb['mm'] = 1000
    gsi = scaffold_half(gdb, stb, b2l)
    relevant = set(gsi['genome'])
    rel_scaffolds = {s for s, g in stb.items() if g in relevant}
    mms = [1000] if skip_mm_profiling else sorted({int(m) for s, c in covT.items() if s in rel_scaffolds for m in c})
    mdb = pd.merge(gsi, coverage_half(covT, stb, s2l, relevant, mms, mask_edges), on=['genome', 'mm'], how='outer')
    if len(ldb) > 0:
        ldb = ldb.copy()
        if skip_mm_profiling:
            ldb = ldb.sort_values('mm').drop_duplicates(subset=['scaffold', 'position_A', 'position_B'], keep='last')
            ldb['mm'] = 1000
        ldb['genome'] = ldb['scaffold'].map(stb)
        if ldb['genome'].notna().any():
            mdb = pd.merge(mdb, linkage_half(ldb, mms), on=['genome', 'mm'], how='left')
    else:
        cols = ['SNV_distance_mean', 'd_prime_mean', 'linked_SNV_count', 'r2_mean']
        for c in cols:
            mdb[c] = np.nan
        mdb[cols] = mdb[cols].astype(float)
    if skip_mm_profiling:
        del mdb['mm']
    return mdb


def assert_same_table(got, exp, what=""):
    """row set and order, column order and integer columns exactly; floats within 1e-9 * max(1, |expected|)"""
    got = got[[c for c in got.columns if c not in NOT_COMPARED]].reset_index(drop=True)
    exp = exp[[c for c in exp.columns if c not in NOT_COMPARED]].reset_index(drop=True)
    assert list(got.columns) == list(exp.columns), (what, list(got.columns), list(exp.columns))
    assert len(got) == len(exp), (what, len(got), len(exp))
    for c in exp.columns:
        g, e = got[c].values, exp[c].values
        if e.dtype.kind in "iu" or e.dtype.kind == "O":
            assert g.dtype.kind == e.dtype.kind, (what, c, g.dtype, e.dtype)
            assert (g == e).all(), (what, c, g, e)
        else:
            assert g.dtype.kind == "f", (what, c, g.dtype)
            assert (np.isnan(g) == np.isnan(e)).all(), (what, c, g, e)
            k = ~np.isnan(e)
            assert (np.abs(g[k] - e[k]) <= 1e-9 * np.maximum(1.0, np.abs(e[k]))).all(), (what, c, g, e)


# ---- the device's per-scaffold rows, derived in numpy from stored tables ----
def load_golden_inputs():
    z = np.load(os.path.join(GOLDEN, "genome_info_inputs.npz"))
    names, lengths = [str(x) for x in z["scaffolds"]], [int(x) for x in z["lengths"]]
    stb = {str(a): str(b) for a, b in z["stb"]}
    s2l = {str(a): int(b) for a, b in zip(z["s2l_names"], z["s2l_lengths"])}
    covT = {n: {} for n in names}
    for si, mm, pos, val in z["cov"]:
        covT[names[si]].setdefault(int(mm), ([], []))
        covT[names[si]][int(mm)][0].append(pos)
        covT[names[si]][int(mm)][1].append(val)
    covT = {n: {mm: pd.Series(np.array(v, dtype="int32"), index=np.array(p, dtype=np.int64)) for mm, (p, v) in c.items()} for n, c in covT.items()}
    ldb = pd.read_csv(os.path.join(GOLDEN, "genome_info_linkage.csv"))
    return dict(names=names, lengths=lengths, stb=stb, s2l=s2l, covT=covT, levels=[int(x) for x in z["levels"]], raw=z["raw"], ldb=ldb)


def scaffold_rows(inp):
    """-> (SCAFFOLD_LEVEL_DT, SNV_LEVEL_DT) [n_scaffolds, n_levels] from the stored per-(scaffold, level) integers"""
    names, levels = inp["names"], inp["levels"]
    lv = np.zeros((len(names), len(levels)), dtype=_lib.SCAFFOLD_LEVEL_DT)
    sv = np.zeros((len(names), len(levels)), dtype=_lib.SNV_LEVEL_DT)
    lv["mm"] = np.asarray(levels)[None, :]
    for r in inp["raw"]:
        i, j = int(r["scaffold"]), levels.index(int(r["mm"]))
        lv[i, j]["present"] = 1
        for f in ("nonzero", "sum_cov", "counted", "sum_clon", "counted_rarefied", "sum_clon_rarefied"):
            lv[i, j][f] = r[f]
        for f in ("divergent", "sns", "snv", "con", "pop"):
            sv[i, j][f] = r[f]
    return lv, sv


def ld_rows(ldb, names, levels):
    """LD_LEVEL_DT [n_scaffolds, n_levels] from a raw linkage table: per level the (A, B) pair's row of the highest mm <= level"""
    out = np.zeros((len(names), len(levels)), dtype=_lib.LD_LEVEL_DT)
    if not len(ldb):
        return out
    sc = ldb["scaffold"].map({n: i for i, n in enumerate(names)}).values
    a, b, mm = ldb["position_A"].values, ldb["position_B"].values, ldb["mm"].values
    r2, dp = ldb["r2"].values.astype(np.float64), ldb["d_prime"].values.astype(np.float64)
    for j, level in enumerate(levels):
        best = {}
        for k in np.flatnonzero(mm <= level):
            key = (sc[k], a[k], b[k])
            if key not in best or mm[best[key]] < mm[k]:
                best[key] = k
        for (s, _, _), k in sorted(best.items()):
            o = out[int(s), j]
            o["n"] += 1
            o["sum_distance"] += int(b[k]) - int(a[k])
            if r2[k] == r2[k]:
                o["n_r2"] += 1
                o["sum_r2"] += r2[k]
            if dp[k] == dp[k]:
                o["n_dprime"] += 1
                o["sum_dprime"] += dp[k]
    return out


def coverage_rows(covT, s2l, names, scaffold_genome, n_genomes, levels, mask_edges=100, hist_bins=None):
    """(GENOME_COV_DT [n_genomes, n_levels], hist [n_genomes, n_levels, bins]) of the named scaffolds, as
    engine.Batch.genome_coverage delivers them"""
    covs = [[masked_coverage(covT, s2l, [n for n, g in zip(names, scaffold_genome) if g == gi], mm, mask_edges).astype(np.int64)
             for mm in levels] for gi in range(n_genomes)]
    top = max([int(c.max()) for row in covs for c in row if len(c)] + [0])
    bins = hist_bins or max(top + 1, 2)
    acc = np.zeros((n_genomes, len(levels)), dtype=_lib.GENOME_COV_DT)
    hist = np.zeros((n_genomes, len(levels), bins), dtype=np.uint32)
    for gi, row in enumerate(covs):
        for j, c in enumerate(row):
            acc[gi, j] = (len(c), int(c.sum()), int((c * c).sum()), int(c.max()) if len(c) else 0, 0)
            hist[gi, j] = np.bincount(np.minimum(c, bins - 1), minlength=bins)
    return acc, hist


def coverage_rows_flat(cov_levels, bounds, scaffold_genome, n_genomes, mask_edges=100, hist_bins=None):
    """coverage_rows on arrays: cov_levels [n_levels, n_pos] = the cumulative coverage of every flat position at every level, bounds =
    the scaffold bounds of the flat space, scaffold_genome[s] = genome id or -1 -> (GENOME_COV_DT [n_genomes, n_levels], hist
    [n_genomes, n_levels, bins]); the last bin catches every coverage >= bins - 1"""
    cov_levels = np.asarray(cov_levels, dtype=np.int64)
    keep = np.full(cov_levels.shape[1], -1, dtype=np.int64)           # the genome a position counts for
    for s, g in enumerate(scaffold_genome):
        lo, hi = int(bounds[s]) + mask_edges, int(bounds[s + 1]) - mask_edges
        if g >= 0 and hi > lo:                                          # shorter than twice the mask, or exactly that: nothing counts
            keep[lo:hi] = g
    bins = hist_bins or max(int(cov_levels[:, keep >= 0].max(initial=0)) + 1, 2)
    acc = np.zeros((n_genomes, cov_levels.shape[0]), dtype=_lib.GENOME_COV_DT)
    hist = np.zeros((n_genomes, cov_levels.shape[0], bins), dtype=np.uint32)
    for gi in range(n_genomes):
        for j in range(cov_levels.shape[0]):
            c = cov_levels[j, keep == gi]
            acc[gi, j] = (len(c), int(c.sum()), int((c * c).sum()), int(c.max()) if len(c) else 0, 0)
            hist[gi, j] = np.bincount(np.minimum(c, bins - 1), minlength=bins)
    return acc, hist
