"""Mirror of the read report of inStrain.filter_reads (inStrain/filter_reads.py:201-300, 699-720) and of what reads it
(profile/fasta.py:87-136 filter_fasta, genomeUtilities.py:617-634 _genome_wide_rr).

The per-scaffold tallies, sums and medians come from the front end's sweep over its pair table (engine.BamFile.read_report,
isx_bam_read_report); everything here is arithmetic over one row per scaffold.  Host only: no device, no Context."""
import logging

import numpy as np
import pandas as pd

COUNT_COLUMNS = ["unfiltered_reads", "unfiltered_pairs", "unfiltered_singletons", "unfiltered_priority_reads", "pass_pairing_filter",
                 "pass_min_read_ani", "pass_max_insert", "pass_min_insert", "pass_min_mapq", "filtered_pairs", "filtered_singletons",
                 "filtered_priority_reads"]
# update_tallys adds evaluate_pair's float verdicts to these four (filter_reads.py:373-374): the reference's columns are float64
FLOAT_COUNTS = ("pass_min_read_ani", "pass_max_insert", "pass_min_insert", "pass_min_mapq")
# (column of the table, the row's integer sum it is the mean of); `mistmaches` is the reference's spelling (:257)
MEAN_COLUMNS = [("mean_mistmaches", "sum_mismatches"), ("mean_insert_distance", "sum_insert_distance"), ("mean_mapq_score", "sum_mapq"),
                ("mean_pair_length", "sum_pair_length")]
COLUMNS = ["scaffold"] + COUNT_COLUMNS + [c for c, _ in MEAN_COLUMNS] + ["mean_PID", "median_insert"]


def mapping_info(rows, names, wanted=None):
    """rows: READ_REPORT_DT [n_refs] (BamFile.read_report(), or the shares' rows put together); names: the header's scaffold
    names; wanted: the reference indices that exist for the filter (None = all).  -> the reference's Rdb
    (filter_scaff2pair2info :231-300): `all_scaffolds` first, then one row per wanted scaffold in HEADER order (the reference's
    order is the arrival order of a worker queue).

    The all_scaffolds row is restated literally from :277-295: it is taken over the scaffolds with pass_pairing_filter > 0 only
    (so a scaffold that holds nothing but single reads does not count towards unfiltered_reads there), counts are summed, and
    mean_* AND median_insert are means weighted by pass_pairing_filter, accumulated in row order with Python's sum."""
    rows = np.asarray(rows)
    idx = list(range(len(rows))) if wanted is None else sorted(int(t) for t in wanted)
    r = rows[idx]
    n = r["pass_pairing_filter"]
    table = {"scaffold": [names[t] for t in idx]}
    for c in COUNT_COLUMNS:
        table[c] = r[c].astype(np.float64) if c in FLOAT_COUNTS else r[c].astype(np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for c, s in MEAN_COLUMNS:
            # an integer sum below 2^53 divided once is np.mean's value bit for bit
            table[c] = np.where(n > 0, r[s].astype(np.float64) / n.astype(np.float64), np.nan)
        table["mean_PID"] = np.where(n > 0, r["sum_pid"] / n.astype(np.float64), np.nan)
    table["median_insert"] = np.where(n > 0, r["median_insert"], np.nan)
    Adb = pd.DataFrame(table, columns=COLUMNS)
    CAdb = Adb[Adb["pass_pairing_filter"] > 0]
    total_reads = CAdb["pass_pairing_filter"].sum()
    top = {"scaffold": ["all_scaffolds"]}
    for c in COLUMNS[1:]:
        if c.startswith("mean_") or c.startswith("median_"):
            with np.errstate(divide="ignore", invalid="ignore"):
                top[c] = [np.float64(sum([v * m for v, m in zip(CAdb[c], CAdb["pass_pairing_filter"])])) / np.float64(total_reads)]
        else:
            top[c] = [int(CAdb[c].sum())]
    adb = pd.DataFrame(top, columns=COLUMNS)
    return pd.concat([adb, Adb]).reset_index(drop=True)


def _header_values(kwargs):
    return {"min_read_ani": kwargs.get("min_read_ani", 0.97), "max_insert_relative": kwargs.get("max_insert_relative", 3),
            "min_insert": kwargs.get("min_insert", 50), "min_mapq": kwargs.get("min_mapq", 2),
            "pairing_filter": kwargs.get("pairing_filter", "paired_only")}


def write_mapping_info(RR, location, **kwargs):
    """mapping_info.tsv as the reference writes it (filter_reads.py:699-720): one `# min_read_ani:... max_insert_relative:... ...` line
    with the filter's settings, then the table, tab-separated; an older file at `location` is replaced.  -> the settings (all that
    happens when location is None)"""
    values = _header_values(kwargs)
    if location is not None:
        with open(location, "w") as f:
            f.write("# " + " ".join("%s:%s" % kv for kv in values.items()) + "\n")
            RR.to_csv(f, index=False, sep="\t")
    return values


def genome_wide_rr(rdb, stb):
    """mapping_info -> one row per genome, genomes in sorted order (what genomeUtilities._genome_wide_rr :617-634 and the steps around
    it, :213-222, leave): the all_scaffolds row and the scaffolds the stb does not name take no part; a count column is summed (and keeps
    its dtype), every other column -- median_insert included -- is the plain mean of the genome's scaffolds that have a value, NaN
    when none has.  Columns: `reads_<column>`, but `filtered_read_pair_count` for filtered_pairs and nothing for pass_pairing_filter.
    One stable sort by genome; the counts are segment sums, the means one numpy mean per genome and column."""
    per = rdb[rdb["scaffold"] != "all_scaffolds"]
    genome = per["scaffold"].map(stb)
    named = genome.notna().values
    per = per[named]
    genomes, gid = np.unique(genome.values[named].astype(object), return_inverse=True)
    order = np.argsort(gid, kind="stable")
    first = np.searchsorted(gid[order], np.arange(len(genomes)))
    bounds = np.r_[first, len(order)]
    out = {"genome": genomes}
    for c in per.columns:
        if c in ("scaffold", "pass_pairing_filter"):
            continue
        v = per[c].values[order]
        if c in COUNT_COLUMNS:
            out["filtered_read_pair_count" if c == "filtered_pairs" else "reads_" + c] = np.add.reduceat(v, first) if len(v) else v[:0]
            continue
        mean = np.full(len(genomes), np.nan)
        for g in range(len(genomes)):
            x = v[bounds[g]:bounds[g + 1]]
            x = x[~np.isnan(x)]
            if len(x):
                mean[g] = x.mean()
        out["reads_" + c] = mean
    return pd.DataFrame(out)


def filter_scaffolds(names, scaffold2pairs, scaffold2length, readlength, min_scaffold_reads=0, min_genome_coverage=0, stb=None):
    """filter_fasta + _filter_genome_coverage (profile/fasta.py:87-136) over scaffold names instead of a split table.
    names: the scaffolds of the run; scaffold2pairs: the report's filtered_pairs; readlength: the all_scaffolds row's
    mean_pair_length (controller.py:265-266).  A genome whose sum(filtered_pairs) * readlength / sum(length) is below
    min_genome_coverage goes with all its scaffolds, and so does every scaffold the stb does not name; then the scaffolds with
    fewer than min_scaffold_reads filtered pairs go.  -> (kept names in the order given, {removed name: reason}).
    (The reference also sorts the survivors by read count; the order here stays the caller's -- no table depends on it.)"""
    names = list(dict.fromkeys(names))
    removed = {}
    if min_genome_coverage > 0:
        if stb is None:
            raise ValueError("If you adjust the minimum genome coverage, you need to provide an .stb!")
        pairs, length = {}, {}
        for s in names:
            g = stb.get(s)
            if g is None:
                continue
            pairs[g] = pairs.get(g, 0) + scaffold2pairs[s]
            length[g] = length.get(g, 0) + scaffold2length[s]
        genome_to_rm = {g for g in pairs if (pairs[g] * readlength) / length[g] < min_genome_coverage}
        rm_1 = {s for s in names if stb.get(s) in genome_to_rm}
        rm_2 = {s for s in names if stb.get(s) is None}
        logging.info("{0} of {1} genomes have less than {2}x estimated coverage".format(len(genome_to_rm), len(pairs), min_genome_coverage))
        logging.info("{0} of the original {1} scaffolds are removed ({2} have a low coverage genome; {3} have no genome)".format(
            len(rm_1 | rm_2), len(names), len(rm_1), len(rm_2)))
        for s in names:
            if s in rm_1:
                removed[s] = "genome {0} has less than {1}x estimated coverage".format(stb[s], min_genome_coverage)
            elif s in rm_2:
                removed[s] = "no genome in the stb"
    kept = []
    for s in names:
        if s in removed:
            continue
        if not scaffold2pairs[s] >= min_scaffold_reads:
            removed[s] = "fewer than {0} filtered read pairs".format(min_scaffold_reads)
        else:
            kept.append(s)
    return kept, removed


def filter_reads(bam, scaffolds=None, threads=0, priority_reads=None, **kwargs):
    """The stand-alone `inStrain filter_reads` (filter_reads.py:82-114, load_paired_reads :157-199): scan, filter and report of
    one BAM -> RR, the mapping_info table.  scaffolds: the names that exist for the filter (the fasta's; None = every reference
    of the header; names the header does not have are ignored, none that it has is a ValueError).  kwargs: min_read_ani, min_mapq, max_insert_relative, min_insert, pairing_filter, with the defaults of
    profile_bam.  Host only."""
    from .. import engine
    bf = engine.BamFile(bam, threads=threads)
    try:
        names = [n for n, _, _ in bf.refs()]
        wanted = None
        if scaffolds is not None:
            keep = set(scaffolds)
            wanted = [t for t, n in enumerate(names) if n in keep]
            if not wanted:                          # (an empty set would mean "every reference" to the handle)
                raise ValueError("filter_reads: none of the given scaffolds is a reference of {0}".format(bam))
        bf.scan()
        if priority_reads:
            bf.set_priority_reads(priority_reads)
        bf.set_wanted_refs(wanted if wanted is not None and len(wanted) < len(names) else [])
        bf.filter(min_read_ani=kwargs.get("min_read_ani", 0.95), min_mapq=kwargs.get("min_mapq", -1),
                  max_insert_relative=kwargs.get("max_insert_relative", 3), min_insert=kwargs.get("min_insert", 50),
                  pairing_filter=kwargs.get("pairing_filter", "paired_only"))
        return mapping_info(bf.read_report(), names, wanted)
    finally:
        bf.close()
