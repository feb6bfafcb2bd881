"""Test-only restatement of the reference's gene rules (inStrain v1.9.1 GeneProfile.py), pandas slice by pandas slice:
characterize_SNPs (:600-707), calc_gene_snp_counts (:495-598), count_sites (:428-486), calc_gene_coverage / calc_gene_clonality
(:352-422) and the merge worker's GeneException (profile_utilities.py:385-396).  The checker of the gene pass; product code never
imports it."""
from collections import defaultdict

import numpy as np
import pandas as pd

_TCAG = "TCAG"
_CODE = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
FORWARD = {a + b + c: _CODE[16 * i + 4 * j + k] for i, a in enumerate(_TCAG) for j, b in enumerate(_TCAG) for k, c in enumerate(_TCAG)}
STOPS = {c for c, aa in FORWARD.items() if aa == '*'}
COMP = {'A': 'T', 'T': 'A', 'C': 'G', 'G': 'C', 'N': 'N'}


def revcomp(s):
    return ''.join(COMP[c] for c in reversed(s))


def translate_codon(codon):
    """Biopython's Standard table on A/C/G/T/N: one amino acid over every expansion -> it; stops only -> '*'; stops and amino
    acids -> 'X'; several amino acids -> B / Z / J when they fit, else 'X'"""
    opts = ['']
    for ch in codon:
        opts = [o + x for o in opts for x in ('ACGT' if ch == 'N' else ch)]
    aas = {FORWARD[o] for o in opts}
    if '*' in aas:
        return '*' if aas == {'*'} else 'X'
    if len(aas) == 1:
        return aas.pop()
    for letter, group in (('B', 'DN'), ('Z', 'EQ'), ('J', 'IL')):
        if aas <= set(group):
            return letter
    return 'X'


def translate(seq):
    return ''.join(translate_codon(seq[i:i + 3]) for i in range(0, len(seq) - len(seq) % 3, 3))


def count_sites(seq):
    S_site = N_site = 0.0
    for i in range(0, len(seq) - len(seq) % 3, 3):
        codon = seq[i:i + 3]
        if 'N' in codon or codon in STOPS:
            continue
        aa = FORWARD[codon]
        s = n = 0
        for p in range(3):
            for b in 'ATCG':
                if b == codon[p]:
                    continue
                nb = codon[:p] + b + codon[p + 1:]
                if nb in STOPS or FORWARD[nb] != aa:
                    n += 1
                else:
                    s += 1
        norm = (n + s) / 3
        S_site += float(s) / float(norm)
        N_site += float(n) / float(norm)
    return S_site, N_site


def characterize_snps(gdb, Sdb, gene2sequence):
    table = defaultdict(list)
    for _, row in Sdb.iterrows():
        db = gdb[(gdb['start'] <= row['position']) & (gdb['end'] >= row['position'])]
        table['position'].append(row['position'])
        if len(db) == 0:
            table['mutation_type'].append('I'); table['mutation'].append(''); table['gene'].append('')
        elif len(db) > 1:
            table['mutation_type'].append('M'); table['mutation'].append(''); table['gene'].append(','.join(db['gene'].tolist()))
        else:
            gene = db['gene'].tolist()[0]
            minus = db['direction'].tolist()[0] == '-1'
            orig = gene2sequence[gene]
            if minus:
                orig = revcomp(orig)
            k = int(row['position'] - db['start'].tolist()[0])
            new = list(orig)
            new[k] = row['con_base']
            if new[k] == orig[k]:
                new[k] = row['var_base']
            new = ''.join(new)
            old_aa = translate(revcomp(orig) if minus else orig)
            new_aa = translate(revcomp(new) if minus else new)
            mut_type, mut = 'S', 'S:' + str(k)
            for i in range(len(old_aa)):
                if new_aa[i] != old_aa[i]:
                    mut_type, mut = 'N', 'N:' + old_aa[i] + str(k) + new_aa[i]
                    break
            table['mutation_type'].append(mut_type); table['mutation'].append(mut); table['gene'].append(gene)
    return pd.DataFrame(table)


def characterize_wrapper(Ldb, gdb, gene2sequence):
    if len(Ldb) == 0:
        return pd.DataFrame()
    Sdb = Ldb.sort_values(['position', 'mm']).drop_duplicates(subset=['scaffold', 'position'], keep='last').sort_index().drop(columns=['mm'])
    Sdb['position'] = Sdb['position'].astype(int)
    Sdb['allele_count'] = Sdb['allele_count'].astype(int)
    Sdb = Sdb[(Sdb['allele_count'] > 0) & (Sdb['allele_count'] <= 2)]
    if len(Sdb) == 0:
        return pd.DataFrame()
    sdb = characterize_snps(gdb, Sdb, gene2sequence)
    return pd.merge(Sdb, sdb, on=['position'], how='left').reset_index(drop=True)


def calc_gene_snp_counts(gdb, ldb, sdb, gene2sequence):
    if len(ldb) == 0:
        return pd.DataFrame()
    xdb = pd.merge(ldb, sdb[['position', 'mutation_type', 'gene']], on=['position'], how='left').reset_index(drop=True)
    sites = {g: count_sites(gene2sequence[g]) for g in gdb['gene']}
    table = defaultdict(list)
    for mm in sorted(xdb['mm'].unique()):
        fdb = xdb[xdb['mm'] <= mm].sort_values('mm', kind='stable').drop_duplicates(subset=['scaffold', 'position'], keep='last')\
            .sort_values('position').set_index('position')
        for _, row in gdb.iterrows():
            db = fdb.loc[int(row['start']):int(row['end'])]
            table['mm'].append(mm); table['gene'].append(row['gene'])
            table['gene_length'].append(abs(row['end'] - row['start']) + 1)
            table['divergent_site_count'].append(len(db))
            for ac, name in zip([1, 2], ['SNS', 'SNV']):
                table[name + '_count'].append(len(db[db['allele_count'] == ac]))
                for t in ['N', 'S']:
                    table['%s_%s_count' % (name, t)].append(len(db[(db['allele_count'] == ac) & (db['mutation_type'] == t)]))
    G = pd.DataFrame(table)
    G['S_sites'] = [sites[g][0] for g in G['gene']]
    G['N_sites'] = [sites[g][1] for g in G['gene']]
    for name, a, b in (('dNdS_substitutions', 'SNS_N_count', 'SNS_S_count'), ('pNpS_variants', 'SNV_N_count', 'SNV_S_count')):
        G[name] = [((nC / nS) / (sC / sS)) if (sC > 0 and sS > 0) else np.nan for nC, nS, sC, sS in zip(G[a], G['N_sites'], G[b], G['S_sites'])]
    return G


def snv_tables(cdb, scaff2geneinfo, scaff2gene2sequence, log_lines=None):
    """the SNV half over a whole cumulative SNV table: {'genes_SNP_count', 'SNP_mutation_types'}, scaffold by scaffold in
    scaff2geneinfo order; a scaffold whose calc_gene_snp_counts raises gives no rows (GeneException)"""
    counts, types = [], []
    for scaff, gdb in scaff2geneinfo.items():
        Ldb = cdb[cdb['scaffold'] == scaff]
        g2s = scaff2gene2sequence[scaff]
        sdb = characterize_wrapper(Ldb, gdb, g2s)
        try:
            ldb = calc_gene_snp_counts(gdb, Ldb, sdb, g2s)
        except KeyError:
            if log_lines is not None:
                log_lines.append("DEBUG FAILURE GeneException {0}".format(scaff))
            continue
        if len(ldb):
            counts.append(ldb)
        if len(sdb):
            types.append(sdb)
    return {'genes_SNP_count': pd.concat(counts).reset_index(drop=True) if counts else pd.DataFrame(),
            'SNP_mutation_types': pd.concat(types).reset_index(drop=True) if types else pd.DataFrame()}


def gene_coverage(gdb, covT):
    """calc_gene_coverage: covT = {mm: Series(coverage of that level, index = position)}"""
    table = defaultdict(list)
    counts = pd.Series(dtype='float64')
    for mm in sorted(covT):
        counts = counts.add(covT[mm], fill_value=0)
        if len(counts) == 0:
            continue
        for _, row in gdb.iterrows():
            gcov = counts.loc[int(row['start']):int(row['end'])]
            glen = abs(row['end'] - row['start']) + 1
            table['gene'].append(row['gene']); table['coverage'].append(gcov.sum() / glen)
            table['breadth'].append(len(gcov) / glen); table['mm'].append(mm)
    return pd.DataFrame(table)


def gene_clonality(gdb, clonT):
    """calc_gene_clonality: clonT = {mm: Series(clonality, index = position)}"""
    table = defaultdict(list)
    p2c = {}
    for mm in sorted(clonT):
        p2c.update(clonT[mm].to_dict())
        inds = sorted(p2c)
        cov = pd.Series([p2c[i] for i in inds], index=np.array(inds).astype('int'), dtype='float64')
        if len(cov) == 0:
            continue
        for _, row in gdb.iterrows():
            gcov = cov.loc[int(row['start']):int(row['end'])]
            glen = abs(row['end'] - row['start']) + 1
            table['gene'].append(row['gene']); table['nucl_diversity'].append(1 - gcov.mean())
            table['breadth_minCov'].append(len(gcov) / glen); table['mm'].append(mm)
    return pd.DataFrame(table)
