"""Mirror of inStrain.GeneProfile (v1.9.1) for `inStrain profile -g genes.fna`: the per-gene tables behind gene_info.tsv.

    parse_genes / parse_prodigal_genes          GeneProfile.py:751-811
    profile_genes_from_profile                  GeneProfile.py:304-350 (the four tables of one scaffold)
    SNVprofile.generate('gene_info')            SNVprofile.py:246-280

The work is done by libinstrain_amd.so (isx_genes_*, isx_batch_profile_genes): the coverage half on a batch's device arrays,
the SNV half (mutation types, per-gene SNV counts) and count_sites on the device; this module lays the genes out, names the rows
and gives them the reference's columns and dtypes.

Deviations (gene profiling): GenBank input is refused (it needs Biopython); a gene whose letters are not upper-case
A/C/G/T/N, or whose length differs from end - start + 1, is a ValueError naming the gene (the reference logs such genes and goes on).
"""
import gzip
import logging

import numpy as np
import pandas as pd

from .. import _lib, engine
from . import emitters

GENE_INFO_COLUMNS = ['scaffold', 'gene', 'gene_length', 'coverage', 'breadth', 'breadth_minCov', 'nucl_diversity', 'start', 'end',
                     'direction', 'partial', 'dNdS_substitutions', 'pNpS_variants', 'SNV_count', 'SNV_S_count', 'SNV_N_count',
                     'SNS_count', 'SNS_S_count', 'SNS_N_count', 'divergent_site_count']
SNP_COUNT_COLUMNS = ['mm', 'gene', 'gene_length', 'divergent_site_count', 'SNS_count', 'SNS_N_count', 'SNS_S_count', 'SNV_count',
                     'SNV_N_count', 'SNV_S_count', 'S_sites', 'N_sites', 'dNdS_substitutions', 'pNpS_variants']
TABLE_NAMES = ['genes_coverage', 'genes_clonality', 'genes_SNP_count', 'SNP_mutation_types']
_SNV_CODE = {'A': 0, 'C': 1, 'T': 2, 'G': 3}
_LETTERS = frozenset('ACGTN')
log = logging.getLogger(__name__)


def _fasta_records(path):
    """(id, description, sequence) of every record (Bio.SeqIO 'fasta': id = the header's first word, the lines joined)"""
    opener = gzip.open if path.endswith('.gz') else open
    head, parts = None, []
    with opener(path, 'rt') as f:
        for line in f:
            line = line.rstrip('\r\n')
            if line.startswith('>'):
                if head is not None:
                    yield head.split(None, 1)[0] if head.strip() else '', head, ''.join(parts)
                head, parts = line[1:], []
            elif head is not None:
                parts.append(line.strip())
    if head is not None:
        yield head.split(None, 1)[0] if head.strip() else '', head, ''.join(parts)


def parse_genes(gene_file_loc, **kwargs):
    """GeneProfile.parse_genes: by extension (.fna / .fa prodigal; .gb / .gbk GenBank is not supported here)"""
    loc = gene_file_loc[:-3] if gene_file_loc.endswith('.gz') else gene_file_loc
    if loc[-4:] == '.fna' or loc[-3:] == '.fa':
        return parse_prodigal_genes(gene_file_loc)
    if loc[-3:] == '.gb' or loc[-4:] == '.gbk':
        raise NotImplementedError("GenBank gene files (%s) need Biopython, which this package does not use: "
                                  "give the genes as a prodigal .fna" % gene_file_loc)
    raise ValueError("I dont know how to process {0}".format(gene_file_loc))


def parse_prodigal_genes(gene_fasta):
    """GeneProfile.parse_prodigal_genes -> (scaff2geneinfo: scaffold -> DataFrame[gene, scaffold, direction, partial, start, end]
    with 0-based inclusive coordinates and `direction` a string, scaff2gene2sequence: scaffold -> gene -> str)"""
    scaff2gene2sequence, tables = {}, {}
    for gene, desc, seq in _fasta_records(gene_fasta):
        scaff = "_".join(gene.split("_")[:-1])
        fields = desc.split("#")
        if len(fields) < 4:
            raise ValueError("gene %s: not a prodigal header (start # end # strand): %r" % (gene, desc))
        start, end = int(fields[1].strip()) - 1, int(fields[2].strip()) - 1     # prodigal is 1-based
        if not set(seq) <= _LETTERS:
            raise ValueError("gene %s: letters other than upper-case A/C/G/T/N in its sequence" % gene)
        if (end - start) + 1 != len(seq):
            raise ValueError("gene %s: start=%d end=%d but %d letters (genes need 1-based coordinates with an INCLUSIVE end)"
                             % (gene, start, end, len(seq)))
        t = tables.setdefault(scaff, {k: [] for k in ('gene', 'scaffold', 'direction', 'partial', 'start', 'end')})
        t['gene'].append(gene)
        t['scaffold'].append(scaff)
        t['direction'].append(fields[3].strip())
        t['partial'].append('partial=01' in desc)
        t['start'].append(start)
        t['end'].append(end)
        scaff2gene2sequence.setdefault(scaff, {})[gene] = seq
    return {s: pd.DataFrame(t) for s, t in tables.items()}, scaff2gene2sequence


def genes_table(scaff2geneinfo):
    """the stored `genes_table` (profile_controller.py:147-149): every scaffold's table, concatenated"""
    return pd.concat(list(scaff2geneinfo.values())) if scaff2geneinfo else pd.DataFrame()


class GeneSet:
    """The genes of a run on the device: scaffold by scaffold in the order of scaff2geneinfo, the gene-table order inside one."""

    def __init__(self, ctx, scaff2geneinfo, scaff2gene2sequence):
        self.gdb = dict(scaff2geneinfo)
        self.first, self.last = {}, {}
        names, starts, ends, strands, seqs = [], [], [], [], []
        for scaff, gdb in self.gdb.items():
            self.first[scaff] = len(names)
            for gene, start, end, direction in zip(gdb['gene'], gdb['start'], gdb['end'], gdb['direction']):
                names.append(gene)
                starts.append(int(start))
                ends.append(int(end))
                strands.append(-1 if str(direction) == '-1' else 1)      # the reference reverse-complements on direction == '-1'
                seqs.append(str(scaff2gene2sequence[scaff][gene]))
            self.last[scaff] = len(names)
        self.names = np.array(names, dtype=object)
        self.start, self.end = np.array(starts, np.int64), np.array(ends, np.int64)
        self.length = np.abs(self.end - self.start) + 1
        self.genes = engine.Genes(ctx, self.start, self.end, strands, seqs)
        self._sites = None

    def sites(self):
        if self._sites is None:
            self._sites = self.genes.sites()[0]
        return self._sites

    def call(self, scaffolds, bounds):
        """(gene_first, gene_last) of a call whose flat space holds `scaffolds` at `bounds`"""
        gf = np.array([self.first.get(s, 0) for s in scaffolds], np.int32)
        gl = np.array([self.last.get(s, 0) for s in scaffolds], np.int32)
        return gf, gl

    def close(self):
        self.genes.close()


def _snv_rows(cdb, offsets):
    """cumulative SNV table rows -> (SNV_DT rows in (gpos, mm) order, the table's row numbers in that order)"""
    gpos = cdb['scaffold'].astype(object).map(offsets).to_numpy(np.int64) + cdb['position'].to_numpy(np.int64)
    mm = cdb['mm'].to_numpy(np.int64)
    order = np.lexsort((mm, gpos))
    v = np.zeros(len(cdb), dtype=_lib.SNV_DT)
    v['gpos'], v['mm'] = gpos[order], mm[order]
    v['con_base'] = [_SNV_CODE.get(b, 4) for b in cdb['con_base'].to_numpy()[order]]
    v['var_base'] = [_SNV_CODE.get(b, 4) for b in cdb['var_base'].to_numpy()[order]]
    col = 'morphia' if 'morphia' in cdb.columns else 'allele_count'
    v['allele_count'] = np.clip(cdb[col].to_numpy(np.int64)[order], 0, 255)
    return v, order


def _snp_tables(gs, scaff, rows, mut, cnt, call_first, cdb, log_lines):
    """genes_SNP_count / SNP_mutation_types of one scaffold from its device rows (`rows`: indices into the sorted table)"""
    gdb = gs.gdb[scaff]
    if len(rows) == 0:
        return None, None                       # no SNV rows: coverage and clonality only (calc_gene_snp_counts returns early)
    m = mut[rows['i']]
    keep = m['type'] != 0
    if not keep.any():
        # Characterize_SNPs_wrapper returns an empty frame, calc_gene_snp_counts indexes it -> KeyError -> the merge worker's
        # GeneException: this scaffold gets no gene rows at all (profile_utilities.py:388-396)
        log_lines.append("DEBUG FAILURE GeneException {0}".format(scaff))
        return False, False
    # SNP_mutation_types: the kept rows in the table's own order, every column but mm
    kr = rows[keep]
    km = m[keep]
    o = np.argsort(kr['orig'], kind='stable')
    kr, km = kr[o], km[o]
    sdb = cdb.iloc[kr['orig']].drop(columns=['mm']).copy()
    sdb['position'] = sdb['position'].astype(int)
    col = 'morphia' if 'morphia' in sdb.columns else 'allele_count'
    sdb[col] = sdb[col].astype(int)
    types, muts, genes = [], [], []
    starts, ends = gdb['start'].to_numpy(), gdb['end'].to_numpy()
    for pos, r in zip(sdb['position'].to_numpy(), km):
        t = chr(r['type'])
        types.append(t)
        if t == 'I':
            muts.append(''); genes.append('')
        elif t == 'M':
            muts.append('')
            genes.append(','.join(gdb['gene'].to_numpy()[(starts <= pos) & (ends >= pos)].tolist()))
        else:
            genes.append(gs.names[r['gene']])
            muts.append('N:%s%d%s' % (chr(r['aa_old']), r['k'], chr(r['aa_new'])) if t == 'N' else 'S:%d' % r['k'])
    sdb['mutation_type'], sdb['mutation'], sdb['gene'] = types, muts, genes
    sdb = sdb.reset_index(drop=True)
    # genes_SNP_count: every level of the scaffold's SNV table x every gene
    mms = np.unique(rows['mm'])
    g0, g1 = gs.first[scaff], gs.last[scaff]
    sites = gs.sites()[g0:g1]
    c = cnt[call_first:call_first + (g1 - g0)]                  # [genes, levels]
    out = {k: [] for k in SNP_COUNT_COLUMNS}
    for mm in mms:
        r = c[:, int(mm)]
        out['mm'].append(np.full(g1 - g0, mm, np.int64))
        out['gene'].append(gs.names[g0:g1])
        out['gene_length'].append(gs.length[g0:g1])
        for name, f in (('divergent_site_count', 'divergent'), ('SNS_count', 'sns'), ('SNS_N_count', 'sns_n'), ('SNS_S_count', 'sns_s'),
                        ('SNV_count', 'snv'), ('SNV_N_count', 'snv_n'), ('SNV_S_count', 'snv_s')):
            out[name].append(r[f].astype(np.int64))
        out['S_sites'].append(sites[:, 0])
        out['N_sites'].append(sites[:, 1])
    ggdb = pd.DataFrame({k: np.concatenate(v) for k, v in out.items() if k not in ('dNdS_substitutions', 'pNpS_variants')})
    ggdb['gene'] = ggdb['gene'].astype(object)
    for name, a, b in (('dNdS_substitutions', 'SNS_N_count', 'SNS_S_count'), ('pNpS_variants', 'SNV_N_count', 'SNV_S_count')):
        nC, sC = ggdb[a].to_numpy(np.float64), ggdb[b].to_numpy(np.float64)
        nS, sS = ggdb['N_sites'].to_numpy(), ggdb['S_sites'].to_numpy()
        ok = (sC > 0) & (sS > 0)
        with np.errstate(divide='ignore', invalid='ignore'):
            ggdb[name] = np.where(ok, (nC / nS) / (sC / sS), np.nan)
    return ggdb, sdb


def _layout(gs, cdb, scaffolds):
    """flat space of an SNV table: the gene scaffolds, each as long as its genes and SNV rows reach"""
    reach = cdb.astype({'scaffold': object}).groupby('scaffold')['position'].max().to_dict() if len(cdb) else {}
    lens = [max(int(gs.end[gs.first[s]:gs.last[s]].max(initial=0)), int(reach.get(s, 0))) + 1 for s in scaffolds]
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def profile_snv_table(cumulative_snv_table, genes, ctx=None, log_lines=None):
    """The SNV half of profile_genes_from_profile on a stored cumulative SNV table: {'genes_SNP_count', 'SNP_mutation_types'}.
    `genes` = (scaff2geneinfo, scaff2gene2sequence) or a GeneSet; scaffolds without genes give nothing, a scaffold whose SNV rows
    leave nothing to classify gives nothing either (the reference's GeneException, logged into log_lines)."""
    own_ctx = ctx is None and not isinstance(genes, GeneSet)
    if own_ctx:
        ctx = engine.Context(0)
    gs = genes if isinstance(genes, GeneSet) else GeneSet(ctx, *genes)
    try:
        tables, _ = _snv_half(gs, cumulative_snv_table, log_lines if log_lines is not None else [])
        return tables
    finally:
        if gs is not genes:
            gs.close()
        if own_ctx:
            ctx.close()


def _snv_half(gs, cumulative_snv_table, log_lines, scaffolds=None):
    scaffolds = [s for s in (gs.gdb if scaffolds is None else scaffolds) if s in gs.gdb]
    cdb = cumulative_snv_table.reset_index(drop=True)
    if len(cdb):
        cdb = cdb[cdb['scaffold'].astype(object).isin(set(scaffolds))].reset_index(drop=True)
    if not scaffolds or not len(cdb):                   # no gene scaffold / no SNV rows: no SNP rows (calc_gene_snp_counts returns early)
        return {'genes_SNP_count': pd.DataFrame(columns=SNP_COUNT_COLUMNS), 'SNP_mutation_types': pd.DataFrame()}, set()
    bounds = _layout(gs, cdb, scaffolds)
    offsets = dict(zip(scaffolds, bounds[:-1]))
    v, order = _snv_rows(cdb, offsets)
    n_levels = int(v['mm'].max()) + 1 if len(v) else 1
    gf, gl = gs.call(scaffolds, bounds)
    mut, cnt, _ = gs.genes.profile_snvs(bounds, gf, gl, v, n_levels)
    scaf_of = np.searchsorted(bounds, v['gpos'].astype(np.int64), side='right') - 1
    rows = np.zeros(len(v), dtype=[('i', np.int64), ('orig', np.int64), ('mm', np.int64)])
    rows['i'], rows['orig'], rows['mm'] = np.arange(len(v)), order, v['mm']
    cuts = np.searchsorted(scaf_of, np.arange(len(scaffolds) + 1))
    counts, types, failed = [], [], set()
    call_first = 0
    for j, scaff in enumerate(scaffolds):
        ggdb, sdb = _snp_tables(gs, scaff, rows[cuts[j]:cuts[j + 1]], mut, cnt, call_first, cdb, log_lines)
        call_first += gs.last[scaff] - gs.first[scaff]
        if ggdb is False:
            failed.add(scaff)
        elif ggdb is not None:
            counts.append(ggdb)
            types.append(sdb)
    out = {'genes_SNP_count': pd.concat(counts).reset_index(drop=True) if counts else pd.DataFrame(columns=SNP_COUNT_COLUMNS),
           'SNP_mutation_types': pd.concat(types).reset_index(drop=True) if types else pd.DataFrame()}
    return out, failed


def coverage_tables(gs, scaffolds, cov_rows, flags, mm_values=None):
    """genes_coverage / genes_clonality (calc_gene_coverage / calc_gene_clonality) of a call's device rows: for every scaffold,
    level by level (a level that is a key of the scaffold's covT / clonT and not empty there), the scaffold's genes in order"""
    M = flags.shape[1]
    mm_values = np.arange(M) if mm_values is None else np.asarray(mm_values)
    cov, clon = [], []
    w = 0
    for j, scaff in enumerate(scaffolds):
        g0, g1 = gs.first.get(scaff, 0), gs.last.get(scaff, 0)
        n = g1 - g0
        if not n:
            continue
        r = cov_rows[w:w + n]
        w += n
        names, glen = gs.names[g0:g1], gs.length[g0:g1].astype(np.float64)
        for b in range(M):
            f = int(flags[j, b])
            if not f & _lib.GENE_LEVEL_PRESENT:
                continue
            mm = int(mm_values[b])
            if f & _lib.GENE_COV_ANY:
                cov.append(pd.DataFrame({'gene': names, 'coverage': r[:, b]['sum_cov'].astype(np.float64) / glen,
                                         'breadth': r[:, b]['nonzero'] / glen, 'mm': np.full(n, mm, np.int64)}))
            if f & _lib.GENE_CLON_ANY:
                counted = r[:, b]['counted'].astype(np.float64)
                with np.errstate(divide='ignore', invalid='ignore'):
                    div = np.where(counted > 0, 1 - r[:, b]['sum_clon'] / counted, np.nan)
                clon.append(pd.DataFrame({'gene': names, 'nucl_diversity': div, 'breadth_minCov': counted / glen,
                                          'mm': np.full(n, mm, np.int64)}))
    return ({'genes_coverage': pd.concat(cov).reset_index(drop=True) if cov else pd.DataFrame(columns=['gene', 'coverage', 'breadth', 'mm']),
             'genes_clonality': pd.concat(clon).reset_index(drop=True) if clon else
             pd.DataFrame(columns=['gene', 'nucl_diversity', 'breadth_minCov', 'mm'])})


def profile_batch(batch, gs, scaffolds, bounds, snv_table, mm_values=None, log_lines=None):
    """profile_genes_from_profile for every scaffold of a run batch: the four tables.  snv_table = the batch's scaffolds'
    cumulative SNV table (columns scaffold, position, mm, con_base, var_base, allele_count, ...)."""
    gf, gl = gs.call(scaffolds, bounds)
    cov_rows, flags, _ = batch.profile_genes(gs.genes, bounds, gf, gl)
    tables = coverage_tables(gs, scaffolds, cov_rows, flags, mm_values)
    snp, failed = _snv_half(gs, snv_table, log_lines if log_lines is not None else [], scaffolds)
    tables.update(snp)
    if failed:                                          # a GeneException scaffold keeps none of its gene rows
        names = set()
        for s in failed:
            names.update(gs.names[gs.first[s]:gs.last[s]].tolist())
        for k in ('genes_coverage', 'genes_clonality'):
            tables[k] = tables[k][~tables[k]['gene'].isin(names)].reset_index(drop=True)
    return tables


def profile_genes_stored(ctx, profile, genes, scaffold2length, max_positions=1 << 27, log_lines=None):
    """`inStrain profile_genes -i IS -g genes.fna` (GeneProfile.calculate_gene_metrics on the stored covT / clonT /
    cumulative_snv_table): the five gene tables exactly as profile_bam(gene_tables=) fills them -- genes_table included, the
    GeneException rule of profile_batch kept.  profile: what stored.load_profile returns; genes: a gene file path,
    (scaff2geneinfo, scaff2gene2sequence) or a GeneSet; scaffold2length: name -> length, whose order is the order of the rows.
    Works in chunks of whole scaffolds of at most max_positions flat positions (a longer scaffold goes alone); only scaffolds
    that have genes are packed.  Per chunk: stored.pack_levels -> engine.StoredLevels -> profile_batch."""
    from . import stored
    if isinstance(genes, str):
        genes = parse_genes(genes)
    gs = genes if isinstance(genes, GeneSet) else GeneSet(ctx, *genes)
    log = log_lines if log_lines is not None else []
    try:
        names = [s for s in scaffold2length if s in gs.gdb]
        levels = stored.profile_levels(profile)
        sdb = profile.get("cumulative_snv_table")
        sdb = pd.DataFrame() if sdb is None else sdb
        parts = {k: [] for k in TABLE_NAMES}
        for cn, _, pack, st in stored.level_chunks(ctx, profile, names, [scaffold2length[s] for s in names], levels, max_positions):
            cdb = sdb[sdb['scaffold'].astype(object).isin(set(cn))] if len(sdb) else sdb
            gt = profile_batch(st, gs, cn, pack["bounds"], cdb, np.asarray(levels, dtype=np.int64), log)
            for k in TABLE_NAMES:
                parts[k].append(gt[k])
        out = {'genes_table': genes_table(gs.gdb)}
        for k in TABLE_NAMES:
            kept = [d for d in parts[k] if len(d)]
            out[k] = pd.concat(kept).reset_index(drop=True) if kept else pd.DataFrame()
        return out
    finally:
        if gs is not genes:
            gs.close()


def gene_info(tables, genes_table):
    """SNVprofile.generate('gene_info'): the highest-mm row of every gene from genes_coverage, genes_clonality and genes_SNP_count
    joined onto genes_table, without N_sites / S_sites, columns ordered, genes with coverage > 0"""
    Gdb = genes_table
    for thing in ['genes_coverage', 'genes_clonality', 'genes_SNP_count']:
        db = tables.get(thing)
        if db is None or len(db) == 0:
            continue
        db = db.sort_values('mm').drop_duplicates(subset=['gene'], keep='last')
        del db['mm']
        Gdb = pd.merge(Gdb, db, on='gene', how='left')
    db = Gdb
    for c in ['N_sites', 'S_sites']:
        if c in db.columns:
            del db[c]
    if len(db) > 0:
        columns = set(db.columns)
        db = db[[c for c in GENE_INFO_COLUMNS if c in columns] + sorted(columns - set(GENE_INFO_COLUMNS))]
        if 'coverage' in db.columns:
            db = db[db['coverage'] > 0]
    return db


def store_tables(tables, genes_table_df, loc):
    """write the tables under the reference's attribute names (SNVprofile raw_data: <loc>/<name>.csv.gz)"""
    import os
    out = {}
    for name, df in list(tables.items()) + [('genes_table', genes_table_df)]:
        out[name] = emitters.store_pandas(df, os.path.join(loc, name))
    return out


def start_genes(ctx, kwargs):
    """profile_bam(gene_file= | genes=(scaff2geneinfo, scaff2gene2sequence)): the run's GeneSet, or None when no genes were asked for"""
    genes = kwargs.get('genes')
    if genes is None and kwargs.get('gene_file'):
        genes = parse_genes(kwargs['gene_file'])
    if genes is None:
        return None
    gs = GeneSet(ctx, *genes)
    gs.tables = {k: [] for k in TABLE_NAMES}
    return gs


def finish_genes(gs, gene_tables):
    """the run's tables into gene_tables (like the reference's gen_snv_profile + genes_table, profile_utilities.py:686-694)"""
    gene_tables['genes_table'] = genes_table(gs.gdb)
    for k in TABLE_NAMES:
        parts = [d for d in gs.tables[k] if len(d)]
        gene_tables[k] = pd.concat(parts).reset_index(drop=True) if parts else pd.DataFrame()
