"""Mirror of inStrain.genomeUtilities (/root/reference/inStrain/genomeUtilities.py).

genome_level_rows: the coverage half of genomeLevel_coverage_info (:297-365) -- per genome and mm level the median / SEM / std of
the coverage of the genome's scaffolds laid end to end with masked scaffold edges (generate_genome_coverage_array :932-981) -- from
the device's per-genome aggregates of ONE batch whose genomes are consecutive scaffolds (engine.Batch.summarize_genomes).

GenomeTables: the whole genome-level table, genomeLevel_from_IS (:145-269), from per-batch device roll-ups that only ever ADD
(engine.Batch.summarize / genome_coverage, engine.snv_level_counts / ld_level_sums), so a genome may be any subset of the scaffolds
and may span batches.  iRep comes from the device too (engine.IRep, finished once per run): set_irep() takes its rows."""
import numpy as np
import pandas as pd

from .._lib import GENOME_COV_DT, IREP_EMPTY, LD_LEVEL_DT, SNV_LEVEL_DT


def genome_level_rows(levels, genomes, mms=None):
    """levels: [n_genomes, n_mm_bins] GENOME_LEVEL_DT from the device; genomes: names in the same order; mms: the levels to
    report (default: all bins; a level beyond the last bin repeats the last one -- coverage is cumulative over levels <= mm)"""
    n_bins = levels.shape[1]
    mms = list(range(n_bins)) if mms is None else [int(m) for m in mms]
    table = {"mm": [], "genome": [], "coverage_median": [], "coverage_SEM": [], "coverage_std": []}
    for g, genome in enumerate(genomes):
        for mm in mms:
            r = levels[g, min(mm, n_bins - 1)]
            n = int(r["n"])
            table["mm"].append(mm)
            table["genome"].append(genome)
            if n == 0:                              # the reference: covs = pd.Series([0])
                med, sem, std = 0, np.nan, 0.0
            else:
                s, q = int(r["sum_cov"]), int(r["sumsq_cov"])
                ss = (n * q - s * s) / n            # sum of squared deviations, from exact integers
                med = int(r["median_cov"])
                std = float(np.sqrt(ss / n))
                sem = float(np.sqrt(ss / (n - 1)) / np.sqrt(n)) if n > 1 else np.nan
            table["coverage_median"].append(med)
            table["coverage_SEM"].append(sem)
            table["coverage_std"].append(std)
    db = pd.DataFrame(table)
    db["iRep"] = np.nan
    db["iRep_GC_corrected"] = np.nan
    return db


def parse_stb(stb):
    """scaffold -> genome from a two-column tab-separated file (genomeUtilities.parse_stb :891-902); a dict is taken as it is.
    (The other forms load_scaff2bin accepts -- .fasta files, no input at all -- are not supported.)"""
    if isinstance(stb, dict):
        return stb
    out = {}
    with open(stb, "r") as ins:
        for line in ins:
            words = line.strip().split('\t')
            scaffold, b = words[:2]
            out[scaffold.strip()] = b.strip()
    return out


def estimate_breadth(coverage):
    """profile_utilities.py:548-555"""
    return (-1) * np.exp(-1 * ((0.883) * coverage)) + 1


def _order_statistic(cum, k):
    """value of the k-th smallest (0-based) of every distribution: cum[..., bins] = cumulative histogram, k[...]"""
    return (cum > k[..., None]).argmax(axis=-1)


def _fasta_codes(fasta):
    """name -> base codes of a scaffold: `fasta` is a path or a dict name -> sequence"""
    from .. import engine
    if isinstance(fasta, dict):
        seqs = fasta
    else:
        from .gene_profile import _fasta_records
        seqs = {name: seq for name, _, seq in _fasta_records(fasta)}
    return lambda name: engine.encode_seq(str(seqs[name]).upper())


def genome_wide_stored(ctx, profile, stb, scaffold2length, fasta=None, mapping_info=None, skip_mm_profiling=False,
                       max_positions=1 << 27, irep=True, scaffold_tables=None, irep_blocks=None):
    """`inStrain genome_wide -i IS -s stb` (genomeLevel_from_IS :145-269 on the stored covT, scaffold table and raw_linkage_table):
    {"genome_info", "scaffold2bin", "bin2length"} as profile_bam(genome_tables=) returns them.  profile: what stored.load_profile
    returns; scaffold2length: name -> length of the run's scaffolds, all of which are laid out, in chunks of whole scaffolds of at most
    max_positions flat positions (a longer scaffold goes alone; a genome may be cut).  Per chunk: StoredLevels.summarize,
    engine.snv_level_counts on the stored SNV table, engine.ld_level_sums on the stored raw_linkage_table, StoredLevels.genome_coverage,
    IRep.add_stored when `fasta` (a path, or name -> sequence) is given and `irep` is true -- otherwise the iRep columns are NaN --
    then GenomeTables.add_batch.  mapping_info: the run's mapping_info for the reads_* columns.  scaffold_tables: a dict that receives
    every scaffold's cumulative_scaffold_table; irep_blocks: a list that receives IRep.blocks() before the fit."""
    from .. import engine
    from . import stored
    from .profile_utilities import make_coverage_table
    s2l = {n: int(v) for n, v in dict(scaffold2length).items()}
    names = list(s2l)
    genomes = GenomeTables(stb, s2l)
    levels = stored.profile_levels(profile)
    mms = np.asarray(levels, dtype=np.int64)
    acc_irep, irep_index = None, {}
    if fasta is not None and irep:
        i_names, i_lengths, i_genome = genomes.irep_scaffolds()
        if i_names:
            acc_irep = engine.IRep(ctx, i_lengths, i_genome, len(genomes.genomes), mask_edges=genomes.mask_edges)
            irep_index = {name: i for i, name in enumerate(i_names)}
    try:
        ref_of = _fasta_codes(fasta) if acc_irep is not None else None
        for cn, cl, pack, st in stored.level_chunks(ctx, profile, names, [s2l[n] for n in names], levels, max_positions, ref_of):
            sb = pack["bounds"]
            rows, _ = st.summarize(sb)
            rows["mm"] = mms[rows["mm"].astype(np.int64)]
            offsets = dict(zip(cn, sb[:-1].tolist()))
            snv_levels, _ = engine.snv_level_counts(ctx, stored.snv_rows(profile.get("cumulative_snv_table"), offsets, levels), sb, len(levels))
            ld_levels, _ = engine.ld_level_sums(ctx, stored.ld_rows(profile.get("raw_linkage_table"), offsets, levels), sb, len(levels))
            ids, local = genomes.batch_genomes(cn)
            acc = hist = None
            if local:
                acc, hist, _ = st.genome_coverage(sb, ids, len(local), mask_edges=genomes.mask_edges)
            if acc_irep is not None:
                acc_irep.add_stored(st, [irep_index.get(n, -1) for n in cn], genomes.irep_level(mms, len(levels), skip_mm_profiling))
            genomes.add_batch(cn, cl, rows, snv_levels, ld_levels, local, acc, hist, mms=mms)
            if scaffold_tables is not None:
                for j, n in enumerate(cn):
                    scaffold_tables[n] = make_coverage_table(rows[j], cl[j], n, None, snv_levels[j])
        if acc_irep is not None:
            if irep_blocks is not None:
                irep_blocks.append(acc_irep.blocks())
            genomes.set_irep(acc_irep.finish()[0])
        if mapping_info is not None:
            genomes.set_mapping_info(mapping_info)
        return {"genome_info": genomes.genome_info(skip_mm_profiling=skip_mm_profiling), "scaffold2bin": genomes.stb,
                "bin2length": genomes.bin2length}
    finally:
        if acc_irep is not None:
            acc_irep.close()


class GenomeTables:
    """genome_info of a run, merged batch by batch.

    stb: scaffold -> genome; scaffold2length: the lengths of the run's scaffolds (a scaffold of the stb without one counts in
    true_scaffolds only, prepare_genome_wide :129-139).  add_batch() takes a batch's per-(scaffold, level) device rows and its
    per-genome coverage distribution; genome_info() makes the reference's table.

    iRep / iRep_GC_corrected are NaN until set_irep() brought the finished rows of an engine.IRep built on irep_scaffolds().
    The reads_* / filtered_read_pair_count columns are there once set_mapping_info() brought the run's mapping_info."""

    def __init__(self, stb, scaffold2length, mask_edges=100):
        self.stb = parse_stb(stb)
        self.s2l = dict(scaffold2length)
        self.mask_edges = int(mask_edges)
        self.genomes = list(dict.fromkeys(self.stb.values()))           # calc_bin2scaffols' order
        self.gidx = {g: i for i, g in enumerate(self.genomes)}
        G = len(self.genomes)
        self.bin2length = {g: 0 for g in self.genomes}
        self.true_scaffolds = np.zeros(G, dtype=np.int64)
        for sc, g in self.stb.items():
            self.true_scaffolds[self.gidx[g]] += 1
            if sc in self.s2l:
                self.bin2length[g] += int(self.s2l[sc])
        self.mms = None                     # the run's levels (mm of device level i), the same for every batch
        self._rows = []                     # per batch: (genome of the row's scaffold or -1, scaffold id, length, level rows, snv rows)
        self._n_scaffolds = 0
        self._seen = set()
        self._ld = None                     # [G + 1, n_levels] LD_LEVEL_DT; the last row collects scaffolds the stb does not name
        self._acc = None                    # [G, n_levels] GENOME_COV_DT
        self._hist = None                   # [G, n_levels, bins] int64
        self._irep = None                   # [G] IREP_ROW_DT (set_irep) or None: both iRep columns NaN
        self._rr = None                     # per genome: the reads_* columns (set_mapping_info) or None: genome_info has none

    def batch_genomes(self, names):
        """-> (genome id of every scaffold for engine.Batch.genome_coverage, -1 = none; the genomes those ids stand for).
        Only scaffolds the stb names AND that have a length take part in a genome's coverage (genomeUtilities.py:312)."""
        local, ids = {}, np.full(len(names), -1, dtype=np.int32)
        for i, sc in enumerate(names):
            g = self.stb.get(sc)
            if g is not None and sc in self.s2l:
                ids[i] = local.setdefault(g, len(local))
        return ids, list(local)

    def irep_scaffolds(self):
        """-> (names, lengths, genome index) of the scaffolds an engine.IRep of this run is built on: those the stb names AND that
        have a length (genomeUtilities.py:312), in the stb's order -- the order ties between equal lengths fall back to"""
        names = [sc for sc in self.stb if sc in self.s2l]
        return (names, np.array([int(self.s2l[sc]) for sc in names], dtype=np.int64),
                np.array([self.gidx[self.stb[sc]] for sc in names], dtype=np.int32))

    def irep_level(self, mms, n_levels, skip_mm_profiling=False):
        """the `level` of engine.IRep.add for a batch of n_levels device levels whose real mm values are mms (None: the ranks):
        the highest level whose mm is <= 1 (maxMM == 1, genomeUtilities.py:331-334), the last one under skip_mm_profiling, -1 = none"""
        if skip_mm_profiling:
            return int(n_levels) - 1
        mms = np.arange(n_levels, dtype=np.int64) if mms is None else np.asarray(mms, dtype=np.int64)
        return int(np.searchsorted(mms, 1, side="right")) - 1

    def set_irep(self, rows):
        """rows: IREP_ROW_DT [n_genomes] of engine.IRep.finish(), genomes in self.genomes' order"""
        rows = np.asarray(rows)
        if rows.shape != (len(self.genomes),):
            raise ValueError("GenomeTables.set_irep: one row per genome expected")
        self._irep = rows.copy()

    def set_mapping_info(self, rdb):
        """rdb: the run's mapping_info (filter_reads.mapping_info).  genome_info() then carries the reference's reads_* columns and
        filtered_read_pair_count (filter_reads.genome_wide_rr, a left merge on `genome`), after the coverage columns and before the
        linkage columns, where genomeLevel_from_IS puts them (:213-228)"""
        from . import filter_reads
        self._rr = filter_reads.genome_wide_rr(rdb, self.stb)

    def irep_accessory(self):
        """one row per genome with the keys of the reference's accessory dict (irep_utilities.py:33-66)"""
        if self._irep is None:
            raise ValueError("GenomeTables.irep_accessory: no iRep rows were set")
        r = self._irep
        flag = np.where((r["flags"] & IREP_EMPTY) != 0, np.nan, 1.0)
        return pd.DataFrame({"genome": self.genomes, "kept_windows": r["kept_windows"], "avg_cov": r["avg_cov"], "r2": r["r2"],
                             "fragMbp": r["fragMbp"], "unfiltered_raw_iRep": r["raw_irep"],
                             "iRep_GC_corrected": pd.Series([np.nan if np.isnan(f) else True for f in flag], dtype=object),
                             "unfiltered_iRep": r["gc_irep"]})

    def _levels(self, mms, n):
        mms = np.arange(n, dtype=np.int64) if mms is None else np.asarray(mms, dtype=np.int64)
        if len(mms) != n:
            raise ValueError("GenomeTables.add_batch: %d levels named for rows of %d levels" % (len(mms), n))
        if self.mms is None:
            self.mms = mms
            L, G = len(mms), len(self.genomes)
            self._ld = np.zeros((G + 1, L), dtype=LD_LEVEL_DT)
            self._acc = np.zeros((G, L), dtype=GENOME_COV_DT)
            self._hist = np.zeros((G, L, 2), dtype=np.int64)
        elif not np.array_equal(self.mms, mms):
            raise ValueError("GenomeTables.add_batch: every batch of a run has the same mm levels")

    def add_batch(self, names, lengths, levels, snv_levels=None, ld_levels=None, genomes=None, acc=None, hist=None, mms=None):
        """names / lengths: the batch's scaffolds; levels [n_scaffolds, n_levels] SCAFFOLD_LEVEL_DT (only rows with `present` count);
        snv_levels SNV_LEVEL_DT and ld_levels LD_LEVEL_DT of the same shape; genomes + acc [n, n_levels] GENOME_COV_DT + hist
        [n, n_levels, bins]: the batch's coverage distribution for the genomes batch_genomes() named; mms: the mm of level i
        (default i).  Everything is added to what earlier batches brought."""
        levels = np.asarray(levels)
        n_sc, L = levels.shape
        self._levels(mms, L)
        if len(names) != n_sc or len(lengths) != n_sc:
            raise ValueError("GenomeTables.add_batch: one name and one length per scaffold row")
        gen = np.array([self.gidx.get(self.stb.get(sc), -1) for sc in names], dtype=np.int64)
        snv = np.zeros((n_sc, L), dtype=SNV_LEVEL_DT) if snv_levels is None else np.asarray(snv_levels)
        sid = np.arange(self._n_scaffolds, self._n_scaffolds + n_sc)
        self._n_scaffolds += n_sc
        self._seen.update(names)
        self._rows.append((gen, sid, np.asarray(lengths, dtype=np.int64), levels, snv))
        if ld_levels is not None:
            ld = np.asarray(ld_levels)
            tgt = np.where(gen >= 0, gen, len(self.genomes))
            for f in LD_LEVEL_DT.names:
                np.add.at(self._ld[f], tgt, ld[f])
        if acc is not None and len(genomes or []):
            g = np.array([self.gidx[x] for x in genomes], dtype=np.int64)
            acc, hist = np.asarray(acc)[:len(g)], np.asarray(hist)[:len(g)]
            if (acc["max_cov"].astype(np.int64) >= hist.shape[-1]).any():
                raise ValueError("GenomeTables.add_batch: a histogram is not exact (max_cov >= its bins); use engine.Batch.genome_coverage")
            if hist.shape[-1] > self._hist.shape[-1]:                   # histograms of different lengths: pad the shorter
                self._hist = np.concatenate([self._hist, np.zeros(self._hist.shape[:2] + (hist.shape[-1] - self._hist.shape[-1],), np.int64)], axis=-1)
            self._hist[g, :, :hist.shape[-1]] += hist
            for f in ("n", "sum_cov", "sumsq_cov"):
                self._acc[f][g] += acc[f].astype(self._acc[f].dtype)
            self._acc["max_cov"][g] = np.maximum(self._acc["max_cov"][g], acc["max_cov"])

    # -- scaffold half (_genomeLevel_scaffold_info_v3 :545-605) --
    def _scaffold_half(self, skip_mm):
        G = len(self.genomes)
        gen = np.concatenate([r[0] for r in self._rows])
        length = np.concatenate([r[2] for r in self._rows]).astype(np.float64)
        lv = np.concatenate([r[3] for r in self._rows])
        snv = np.concatenate([r[4] for r in self._rows])
        present = lv["present"] != 0                                   # [S, L]
        S, L = present.shape
        run_levels = np.flatnonzero(present.any(axis=0))                # levels that are a key of some scaffold's covT
        # forward fill: at level l a scaffold contributes its row of the highest present level <= l
        idx = np.where(present, np.arange(L)[None, :], -1)
        src = np.maximum.accumulate(idx, axis=1)
        if skip_mm:                                                    # every scaffold's last level, as one level `1000`
            src, out_levels, out_mm = src[:, -1:], [0], [1000]
        else:
            src, out_levels, out_mm = src[:, run_levels], range(len(run_levels)), [int(self.mms[l]) for l in run_levels]
        rows = np.arange(S)[:, None]
        ok = (src >= 0) & (gen >= 0)[:, None]
        pick = np.where(src >= 0, src, 0)
        r, v = lv[rows, pick], snv[rows, pick]
        ln = length[:, None]
        w = np.where(ok, 1.0, 0.0)
        g = np.where(gen >= 0, gen, 0)
        b2l = np.array([self.bin2length[x] for x in self.genomes], dtype=np.float64)
        counted, rare = r["counted"].astype(np.float64), r["counted_rarefied"].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            breadth = r["nonzero"].astype(np.float64) / ln
            coverage = r["sum_cov"].astype(np.float64) / ln
            considered = (counted / ln) * ln                             # breadth_minCov * length
            nd = np.where(counted > 0, 1 - r["sum_clon"] / counted, 0.0)         # NaN counts as 0
            ndr = np.where(rare > 0, 1 - r["sum_clon_rarefied"] / rare, 0.0)

        def per_genome(x, dtype=np.float64):
            out = np.zeros((G, x.shape[1]), dtype=dtype)
            np.add.at(out, g, np.where(ok, x, 0).astype(dtype))
            return out

        detected = per_genome(w, np.int64)
        cons = per_genome(considered)
        table = {k: [] for k in ("mm", "genome", "detected_scaffolds", "true_scaffolds", "length", "SNS_count", "SNV_count",
                                 "divergent_site_count", "consensus_divergent_sites", "population_divergent_sites", "breadth", "coverage",
                                 "nucl_diversity", "nucl_diversity_rarefied", "conANI_reference", "popANI_reference", "breadth_minCov",
                                 "breadth_expected")}
        sums = {"SNS_count": per_genome(v["sns"], np.int64), "SNV_count": per_genome(v["snv"], np.int64),
                "divergent_site_count": per_genome(v["divergent"], np.int64), "consensus_divergent_sites": per_genome(v["con"], np.int64),
                "population_divergent_sites": per_genome(v["pop"], np.int64)}
        with np.errstate(divide="ignore", invalid="ignore"):
            g_breadth = per_genome(breadth * ln) / b2l[:, None]
            g_cov = per_genome(coverage * ln) / b2l[:, None]
            g_nd = np.where(cons != 0, per_genome(nd * considered) / cons, np.nan)
            g_ndr = np.where(cons != 0, per_genome(ndr * considered) / cons, np.nan)
            g_con = np.where(cons != 0, (cons - sums["consensus_divergent_sites"]) / cons, 0.0)
            g_pop = np.where(cons != 0, (cons - sums["population_divergent_sites"]) / cons, 0.0)
            g_bmc = cons / b2l[:, None]
        by_name = sorted(range(G), key=lambda i: self.genomes[i])      # groupby('genome') sorts
        for j, mm in zip(out_levels, out_mm):
            for i in by_name:
                if detected[i, j] == 0:
                    continue
                table["mm"].append(mm)
                table["genome"].append(self.genomes[i])
                table["detected_scaffolds"].append(int(detected[i, j]))
                table["true_scaffolds"].append(int(self.true_scaffolds[i]))
                table["length"].append(int(b2l[i]))
                for k, a in sums.items():
                    table[k].append(int(a[i, j]))
                table["breadth"].append(g_breadth[i, j])
                table["coverage"].append(g_cov[i, j])
                table["nucl_diversity"].append(g_nd[i, j])
                table["nucl_diversity_rarefied"].append(g_ndr[i, j])
                table["conANI_reference"].append(g_con[i, j])
                table["popANI_reference"].append(g_pop[i, j])
                table["breadth_minCov"].append(g_bmc[i, j])
                table["breadth_expected"].append(estimate_breadth(g_cov[i, j]))
        # the levels the coverage half reports: the keys of covT over the scaffolds of the genomes found above
        relevant = sorted(set(table["genome"]), key=self.gidx.get)
        rel = np.isin(gen, [self.gidx[x] for x in relevant])
        cov_levels = np.flatnonzero((present & rel[:, None]).any(axis=0))
        return pd.DataFrame(table), relevant, cov_levels

    # -- coverage half (genomeLevel_coverage_info :297-365 without iRep) --
    def _coverage_half(self, relevant, cov_levels, skip_mm):
        acc = {f: self._acc[f].astype(np.int64) for f in ("n", "sum_cov", "sumsq_cov")}
        hist = self._hist.copy()
        for sc, g in self.stb.items():                                  # a scaffold no batch brought: all zeros (covT has no such key)
            if sc in self.s2l and sc not in self._seen and int(self.s2l[sc]) >= 2 * self.mask_edges:
                k = int(self.s2l[sc]) - 2 * self.mask_edges
                acc["n"][self.gidx[g]] += k
                hist[self.gidx[g], :, 0] += k
        levels, mms = ([len(self.mms) - 1], [1000]) if skip_mm else (list(cov_levels), [int(self.mms[l]) for l in cov_levels])
        cum = np.cumsum(hist, axis=-1)
        table = {"mm": [], "genome": [], "coverage_median": [], "coverage_SEM": [], "coverage_std": []}
        for genome in relevant:
            i = self.gidx[genome]
            n_l = acc["n"][i][levels]
            lo = _order_statistic(cum[i][levels], np.maximum(n_l - 1, 0) // 2)
            hi = _order_statistic(cum[i][levels], n_l // 2)
            for j, (l, mm) in enumerate(zip(levels, mms)):
                n = int(n_l[j])
                table["mm"].append(mm)
                table["genome"].append(genome)
                if n == 0:                                              # the reference: covs = pd.Series([0])
                    med, sem, std = 0, np.nan, 0.0
                else:
                    s, q = int(acc["sum_cov"][i, l]), int(acc["sumsq_cov"][i, l])
                    ss = (n * q - s * s) / n                            # sum of squared deviations, from exact integers
                    med = int((int(lo[j]) + int(hi[j])) / 2.0)
                    std = float(np.sqrt(ss / n))
                    sem = float(np.sqrt(ss / (n - 1)) / np.sqrt(n)) if n > 1 else np.nan
                table["coverage_median"].append(med)
                table["coverage_SEM"].append(sem)
                table["coverage_std"].append(std)
        db = pd.DataFrame(table)
        db["iRep"] = np.nan
        db["iRep_GC_corrected"] = np.nan
        # iRep is computed once per genome, at maxMM == 1 (all levels under skip_mm_profiling), and goes into every row of the
        # genome; a table without an mm == 1 row never computes it (genomeUtilities.py:324-361).  The flag is True whenever the
        # computation ran with GC windows, NaN when it raised (an empty genome array)
        if self._irep is not None and len(db) and (skip_mm or 1 in mms):
            gi = np.array([self.gidx[g] for g in db["genome"]], dtype=np.int64)
            db["iRep"] = self._irep["irep"][gi]
            empty = (self._irep["flags"][gi] & IREP_EMPTY) != 0
            db["iRep_GC_corrected"] = pd.Series([np.nan if e else True for e in empty], dtype=object, index=db.index)
        return db, levels, mms

    # -- linkage half (_genome_wide_linkage :636-659) --
    def _linkage_half(self, levels, mms):
        table = {"genome": [], "mm": [], "r2_mean": [], "d_prime_mean": [], "SNV_distance_mean": [], "linked_SNV_count": []}
        ld = self._ld[:-1]
        by_name = sorted(range(len(self.genomes)), key=lambda i: self.genomes[i])
        for l, mm in zip(levels, mms):
            for i in by_name:
                r = ld[i, l]
                if r["n"] == 0:
                    continue
                table["genome"].append(self.genomes[i])
                table["mm"].append(mm)
                table["r2_mean"].append(r["sum_r2"] / r["n_r2"] if r["n_r2"] else np.nan)
                table["d_prime_mean"].append(r["sum_dprime"] / r["n_dprime"] if r["n_dprime"] else np.nan)
                table["SNV_distance_mean"].append(int(r["sum_distance"]) / int(r["n"]))
                table["linked_SNV_count"].append(int(r["n"]))
        return pd.DataFrame(table)

    def genome_info(self, skip_mm_profiling=False):
        """the reference's genome_info table (genomeLevel_from_IS): one row per genome and mm level, or per genome with
        skip_mm_profiling (every scaffold's last level, no mm column); column names, order and dtypes as the reference's; its
        reads_* / filtered_read_pair_count columns only after set_mapping_info() (see the class)."""
        if self.mms is None:
            raise ValueError("GenomeTables.genome_info: no batch was added")
        skip = bool(skip_mm_profiling)
        gsi, relevant, cov_levels = self._scaffold_half(skip)
        eg, levels, mms = self._coverage_half(relevant, cov_levels, skip)
        mdb = pd.merge(gsi, eg, on=["genome", "mm"], how="outer")
        if self._rr is not None:                                        # genomeUtilities.py:228: before the linkage columns
            mdb = pd.merge(mdb, self._rr, on=["genome"], how="left")
        last = len(self.mms) - 1
        if int(self._ld["n"][:, last].sum()) > 0:                       # the run has linkage rows
            if int(self._ld["n"][:-1, last].sum()) > 0:                 # ... on scaffolds of the stb
                mdb = pd.merge(mdb, self._linkage_half(levels, mms), on=["genome", "mm"], how="left")
        else:
            cols = ["SNV_distance_mean", "d_prime_mean", "linked_SNV_count", "r2_mean"]
            for c in cols:
                mdb[c] = np.nan
            mdb[cols] = mdb[cols].astype(float)
        if skip:
            del mdb["mm"]
        return mdb
