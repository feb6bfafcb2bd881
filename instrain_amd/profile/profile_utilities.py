"""Mirror of inStrain/profile/profile_utilities.py for the hot path: profile_split's result carrier
(SplitObject, profile_utilities.py:823-858 and the fields set at :195-211), the scaffold_profile the merge
step builds from it (:860-896), and the batch driver that replaces the split worker pool
(profile_controller.py:157-271, 397-457).

profile_bam keeps the reference's contract (profile/__init__.py:7-18):
  * `fasta_db` (scaffold, split_number, start, end) decides which scaffolds / splits are profiled
    (profile_controller.py:415-433); without it every reference of the BAM that has a sequence is;
  * `sR2M` (scaffold -> {pair: mm} or set of pairs, controller.py:274-281) decides which read pairs count and
    with which mm; without it the built-in read filter (filter_reads.py) runs with the flags in kwargs;
  * a scaffold that cannot be profiled (not in the BAM, no / wrong sequence, a failing batch) is logged with the
    reference's "SplitException" line and dropped -- the others go on (profile_utilities.py:100-111, 154-156).
"""
import functools
import logging
import os
import time
import traceback
import types

import numpy as np
import pandas as pd

from .. import dist as idist
from .. import _lib, engine
from . import filter_reads, gene_profile, genome_utilities
from .snv_utilities import CLASSES, null_model_lut

BASES = np.array(["A", "C", "T", "G", "N"])
LD_COLUMNS = ['r2', 'd_prime', 'r2_normalized', 'd_prime_normalized', 'total', 'countAB', 'countAb', 'countaB',
              'countab', 'allele_A', 'allele_a', 'allele_B', 'allele_b', 'distance', 'position_A', 'position_B',
              'mm', 'scaffold']          # linkage.py:230-249 + calculate_ld :67-71
SNP_COLUMNS = ['scaffold', 'position', 'ref_base', 'A', 'C', 'T', 'G', 'con_base', 'var_base', 'mm',
               'allele_count', 'class', 'cryptic', 'position_coverage']   # snv_utilities.py:118-127, 274-290
COVERAGE_COLUMNS = ['scaffold', 'length', 'breadth', 'coverage', 'coverage_median', 'coverage_std', 'coverage_SEM',
                    'nucl_diversity', 'nucl_diversity_median', 'nucl_diversity_rarefied', 'nucl_diversity_rarefied_median',
                    'breadth_minCov', 'breadth_rarefied', 'breadth_expected', 'divergent_site_count', 'SNS_count',
                    'SNV_count', 'consensus_divergent_sites', 'population_divergent_sites', 'conANI_reference',
                    'popANI_reference', 'mm']


def iterate_splits(sLen, window_length=10000):
    """fasta.py:56-73"""
    from ..synth import iterate_splits as it
    return it(sLen, window_length)


# ---------------------------------------------------------------------------------------------------------
# result carriers
# ---------------------------------------------------------------------------------------------------------
_COPIERS = None


def _own(a):
    """a numpy array that stays valid after the pipe slot it may point into is released (a position-sized table of a metagenome batch
    is hundreds of MB: pieces are copied side by side -- numpy's copy loop runs without the GIL)"""
    if a.flags.owndata or isinstance(a.base, np.ndarray) and a.base.flags.owndata:
        return a
    if a.nbytes < (16 << 20) or not a.flags.c_contiguous:
        return np.array(a)
    global _COPIERS
    if _COPIERS is None:
        from concurrent.futures import ThreadPoolExecutor
        _COPIERS = ThreadPoolExecutor(6)
    out = np.empty_like(a)
    n = len(a)
    step = -(-n // 12)
    list(_COPIERS.map(lambda k: np.copyto(out[k:k + step], a[k:k + step]), range(0, n, step)))
    return out


def _cuts(col, bounds):
    """np.searchsorted(col, bounds) for a column of a structured array: numpy would first copy the strided column
    (hundreds of MB for an entry table), a bisection only touches len(bounds) * log2(len(col)) of its elements"""
    n = len(col)
    lo = np.zeros(len(bounds), dtype=np.int64)
    hi = np.full(len(bounds), n, dtype=np.int64)
    b = np.asarray(bounds, dtype=np.int64)
    while True:
        act = lo < hi
        if not act.any():
            return lo
        mid = (lo + hi) >> 1
        v = col[np.minimum(mid, max(n - 1, 0))].astype(np.int64) if n else b
        right = act & (v < b)
        lo = np.where(right, mid + 1, lo)
        hi = np.where(act & ~right, mid, hi)


class _BatchTables:
    """The tables of one device batch, cut per split on demand (shrink_basewise / generate_snp_table /
    calculate_ld outputs of every split of the batch).  Built once per batch from numpy arrays; the pandas
    objects of a split are only made when somebody reads them."""

    def __init__(self, res, split_bounds, split_scaffold, scaffold_offset, min_cov=5, mm_values=None):
        self.min_cov = int(min_cov)
        # mm levels beyond what a device batch indexes directly: the device's levels are RANKS, mm_values[rank] the pairs' real mm
        # (profile_bam, isx_bam_set_mm_levels); every mm that leaves this object goes through _mm()
        self.mm_values = None if mm_values is None else np.asarray(mm_values, dtype=np.int64)
        self.bounds = np.asarray(split_bounds, dtype=np.int64)
        self.scaffold = split_scaffold
        self.offset = np.asarray(scaffold_offset, dtype=np.int64)
        self.snv, self.ld = _own(res["snv"]), _own(res["ld"])
        self.s_cut = _cuts(self.snv["gpos"], self.bounds)
        self.l_cut = _cuts(self.ld["gpos_a"], self.bounds)
        self._soa = self.entries = self._lev = self._e_cut = None
        if "level_tables" in res:                   # mm profiling on, level-sparse hand-back (round 6): own copies of the level tables, 1-3 bytes a
            self._lev = res["level_tables"]         # level; the columns below are made from them the first time a split's tables are read
        elif "entries_soa" in res:                  # mm profiling on, shrunk hand-back: columns gpos | mm << 24 | cov | clon | clon_rarefied
            self._soa = res["entries_soa"]
        elif "entries" in res:                      # mm profiling on: (position, mm) entries
            self.entries = res["entries"]
            self._e_cut = _cuts(self.entries["gpos"], self.bounds)
        if self._soa is None and self._lev is None and self.entries is None:       # one mm bin: coverage per position, clonality, sparse clonTR
            if "counts" in res:
                self.cov = res["counts"].sum(axis=1, dtype=np.int64)
            else:                                   # the shrunk hand-back: 16- or 8-bit coverage + the exact values beyond
                self.cov = engine.dense_cov(res) if "cov4" in res else _own(res["cov16"] if "cov16" in res else res["cov8"])
                if res.get("n_saturated"):
                    if "saturated" not in res:
                        raise ValueError("coverage beyond the hand-back's range at too many positions: profile with store_everything")
                    self.cov = self.cov.astype(np.int64)
                    self.cov[res["saturated"]["gpos"]] = res["saturated"]["coverage"]
            if "clon_sparse" in res:                # clonality shrunk: 1.0 wherever the coverage reaches min_cov, except the listed positions
                self.clon = None
                self.clon_pos = res["clon_sparse"]["gpos"].astype(np.int64)
                self.clon_val = np.array(res["clon_sparse"]["clon"])
                self.c_cut = np.searchsorted(self.clon_pos, self.bounds)
            else:
                self.clon = _own(res["clon"])
            self.clon_r = None
            if "rare" in res:
                self.rare_pos = res["rare"]["gpos"].astype(np.int64)
                self.rare_val = np.array(res["rare"]["clon_rarefied"])
                self.r_cut = np.searchsorted(self.rare_pos, self.bounds)
            else:                                   # a deep sample: the dense array, cut per split when somebody asks
                self.clon_r = _own(res["clon_r"])
        self.pileup_counts = _own(res["counts"]) if "counts" in res and self.entries is None and self._soa is None and self._lev is None else None
        if self.pileup_counts is None and self.entries is not None and res.get("allele_obs") is not None:
            # --store_everything with mm profiling on: pileup_counts[pos] = the counts over ALL mm levels (profile_utilities.py:257-259)
            pc = np.zeros((int(self.bounds[-1]), 4), dtype=np.int64)
            np.add.at(pc, self.entries["gpos"].astype(np.int64), self.entries["cnt"].astype(np.int64))
            self.pileup_counts = pc
        # --store_everything: update_linked_reads' appends as the device holds them (read_to_snvs / mm_to_position_graph are
        # made from them per split, profile/linkage.py); pair_names: the batch's dense pair id -> read-pair name
        self.ao = res.get("allele_obs")
        if self.ao is not None and self.mm_values is not None:
            self.ao = self.ao.copy()
            self.ao["mm"] = self._mm(self.ao["mm"])
        if self.ao is not None:                     # sorted by position once: a split cuts its rows by bisection (profile/linkage.py)
            from . import linkage
            self.ao = linkage.SortedAlleleObs(self.ao)
        self.pair_names = res.get("pair_names")

    def _mm(self, levels):
        """device level -> the pairs' mm"""
        levels = np.asarray(levels)
        return levels if self.mm_values is None else self.mm_values[levels.astype(np.int64)]

    @property
    def soa(self):
        if self._soa is None and self._lev is not None:
            self._soa = self._lev.columns()
            self._lev = None
        return self._soa

    @property
    def e_cut(self):
        if self._e_cut is None:
            self._e_cut = _cuts(self.soa[0], self.bounds)
        return self._e_cut

    # -- shrink_basewise (profile_utilities.py:337-350): dict mm -> sparse Series; a level that occurs in the split keeps
    #    its key even when its Series is empty (the reference deletes nothing but zeros / NaNs) --
    def _by_mm(self, pos, mm, val, dtype, all_mm):
        out = {int(m): pd.Series(np.zeros(0, dtype=dtype), index=np.zeros(0, dtype=np.int64)) for m in all_mm}
        if len(pos):
            order = np.lexsort((pos, mm))
            pos, mm, val = pos[order], mm[order], val[order]
            cuts = np.flatnonzero(np.diff(mm)) + 1
            for s, e in zip(np.r_[0, cuts], np.r_[cuts, len(mm)]):
                out[int(mm[s])] = pd.Series(val[s:e].astype(dtype), index=pos[s:e].astype(np.int64))
        return out

    def basewise(self, i):
        """-> covT, clonT, clonTR of split i"""
        off = self.offset[i]
        if self.soa is not None:
            a, b = self.e_cut[i], self.e_cut[i + 1]
            g, mc, cl, cr = (x[a:b] for x in self.soa)
            pos = g.astype(np.int64) - off
            mm, lvl = self._mm((mc >> 24).astype(np.uint16)), (mc & 0xFFFFFF).astype(np.int64)
            all_mm = np.unique(mm)
            k = lvl > 0
            covT = self._by_mm(pos[k], mm[k], lvl[k], "int32", all_mm)
            k = ~np.isnan(cl)
            clonT = self._by_mm(pos[k], mm[k], cl[k], "float32", all_mm)
            k = ~np.isnan(cr)
            clonTR = self._by_mm(pos[k], mm[k], cr[k], "float32", all_mm)
            return covT, clonT, clonTR
        if self.entries is not None:
            ee = self.entries[self.e_cut[i]:self.e_cut[i + 1]]
            pos = ee["gpos"].astype(np.int64) - off
            emm = self._mm(ee["mm"])
            all_mm = np.unique(emm)
            lvl = ee["cnt"].sum(axis=1)
            k = lvl > 0
            covT = self._by_mm(pos[k], emm[k], lvl[k], "int32", all_mm)
            k = ~np.isnan(ee["clon"])
            clonT = self._by_mm(pos[k], emm[k], ee["clon"][k], "float32", all_mm)
            k = ~np.isnan(ee["clon_rarefied"])
            clonTR = self._by_mm(pos[k], emm[k], ee["clon_rarefied"][k], "float32", all_mm)
            return covT, clonT, clonTR
        s, e = int(self.bounds[i]), int(self.bounds[i + 1])
        cov = self.cov[s:e]
        k = np.flatnonzero(cov)
        if len(k) == 0:
            return {}, {}, {}                       # no read reached the split: no mm level was ever created
        covT = {0: pd.Series(cov[k].astype("int32"), index=k + (s - off))}
        if self.clon is None:
            kc = np.flatnonzero(cov >= self.min_cov)
            vals = np.ones(len(kc), dtype="float32")
            c0, c1 = self.c_cut[i], self.c_cut[i + 1]
            if c1 > c0:
                vals[np.searchsorted(kc, self.clon_pos[c0:c1] - s)] = self.clon_val[c0:c1]
            clonT = {0: pd.Series(vals, index=kc + (s - off))}
        else:
            cl = self.clon[s:e]
            k = np.flatnonzero(~np.isnan(cl))
            clonT = {0: pd.Series(cl[k].astype("float32"), index=k + (s - off))}
        if self.clon_r is not None:
            cr = self.clon_r[s:e]
            k = np.flatnonzero(~np.isnan(cr))
            clonTR = {0: pd.Series(cr[k].astype("float32"), index=k + (s - off))}
        else:
            r0, r1 = self.r_cut[i], self.r_cut[i + 1]
            clonTR = {0: pd.Series(self.rare_val[r0:r1].astype("float32"), index=self.rare_pos[r0:r1] - off)}
        return covT, clonT, clonTR

    def snp_table(self, i, i_end=None):
        """raw_snp_table of split i, or of the consecutive splits [i, i_end) of ONE scaffold"""
        snv = self.snv[self.s_cut[i]:self.s_cut[i + 1 if i_end is None else i_end]]
        if not len(snv):
            return pd.DataFrame()
        cnt = snv["cnt"].astype(np.int64)
        return pd.DataFrame({
            'scaffold': self.scaffold[i], 'position': snv["gpos"].astype(np.int64) - self.offset[i],
            'ref_base': BASES[snv["ref_base"]], 'A': cnt[:, 0], 'C': cnt[:, 1], 'T': cnt[:, 2], 'G': cnt[:, 3],
            'con_base': BASES[snv["con_base"]], 'var_base': BASES[snv["var_base"]], 'mm': self._mm(snv["mm"]).astype(np.int64),
            'allele_count': snv["allele_count"].astype(np.int64), 'class': np.array(CLASSES)[snv["cls"]],
            'cryptic': snv["cryptic"].astype(bool), 'position_coverage': cnt.sum(axis=1)}, columns=SNP_COLUMNS)

    def linkage_table(self, i):
        ld = self.ld[self.l_cut[i]:self.l_cut[i + 1]]
        if not len(ld):
            return pd.DataFrame()
        pa = ld["gpos_a"].astype(np.int64) - self.offset[i]
        pb = ld["gpos_b"].astype(np.int64) - self.offset[i]
        return pd.DataFrame({
            'r2': ld["r2"], 'd_prime': ld["d_prime"], 'r2_normalized': ld["r2_normalized"],
            'd_prime_normalized': ld["d_prime_normalized"], 'total': ld["total"].astype(np.int64),
            'countAB': ld["countAB"].astype(np.int64), 'countAb': ld["countAb"].astype(np.int64),
            'countaB': ld["countaB"].astype(np.int64), 'countab': ld["countab"].astype(np.int64),
            'allele_A': BASES[ld["allele_A"]], 'allele_a': BASES[ld["allele_a"]], 'allele_B': BASES[ld["allele_B"]],
            'allele_b': BASES[ld["allele_b"]], 'distance': np.abs(pb - pa), 'position_A': pa, 'position_B': pb,
            'mm': self._mm(ld["mm"]).astype(np.int64), 'scaffold': self.scaffold[i]}, columns=LD_COLUMNS)


class SplitObject():
    '''Holds the profile of an individual split (same attributes as the reference's SplitObject,
    profile_utilities.py:823-858).  covT / clonT / clonTR / raw_snp_table / raw_linkage_table are cut out of the
    batch's tables the first time they are read.'''
    _LAZY = ('covT', 'clonT', 'clonTR', 'raw_snp_table', 'raw_linkage_table', 'pileup_counts', 'read_to_snvs', 'mm_to_position_graph')
    # the plain fields too are read off the batch's split table on first access: a 1000-genome database is tens of thousands of
    # splits a batch, and building every object's strings eagerly was a fifth of profile_bam's time on it
    _META = ('scaffold', 'split_number', 'bam', 'length', 'min_freq', 'log', 'mm_clamped')   # mm_clamped: None, or the level pairs beyond it were merged into

    def __init__(self):
        pass

    @classmethod
    def _of_batch(cls, tables, i):
        S = cls.__new__(cls)
        S.__dict__['_src'] = (tables, i)
        return S

    def __getattr__(self, name):                    # only reached when the attribute is not set yet
        src = self.__dict__.get('_src')
        if src is None or (name not in SplitObject._LAZY and name not in SplitObject._META):
            raise AttributeError(name)
        tables, i = src
        if name in SplitObject._META:
            m = tables.meta
            d = self.__dict__
            d['scaffold'] = m['scaffold'][i]
            d['split_number'] = int(m['number'][i])
            d['bam'] = m['bam']
            d['length'] = int(m['length'][i])
            d['min_freq'] = m['min_freq']
            d['mm_clamped'] = m.get('mm_clamped')
            unit = "{0}.{1}".format(d['scaffold'], d['split_number'])    # profile_utilities.py:133-134, 212-214
            d['log'] = get_worker_log('SplitProfile', unit, 'start', m['t_start'], m['mem']) + get_worker_log('SplitProfile', unit, 'end', m['t_end'], m['mem'])
            return d[name]
        if name in ('covT', 'clonT', 'clonTR'):
            self.covT, self.clonT, self.clonTR = tables.basewise(i)
        elif name == 'raw_snp_table':
            self.raw_snp_table = tables.snp_table(i)
        elif name == 'raw_linkage_table':
            self.raw_linkage_table = tables.linkage_table(i)
        elif name == 'pileup_counts':               # --store_everything (profile_utilities.py:205-211)
            if tables.pileup_counts is None:
                raise AttributeError(name)
            self.pileup_counts = tables.pileup_counts[int(tables.bounds[i]):int(tables.bounds[i + 1])].astype(np.int64)
        elif name in ('read_to_snvs', 'mm_to_position_graph'):      # --store_everything (profile_utilities.py:205-211)
            if tables.ao is None:
                raise AttributeError(name)
            from . import linkage
            self.read_to_snvs = linkage.read_to_snvs_of_split(tables.ao, int(tables.bounds[i]), int(tables.bounds[i + 1]), tables.pair_names)
            self.mm_to_position_graph = linkage.calc_mm_SNV_linkage_network(self.read_to_snvs, scaff=self.scaffold)
        return self.__dict__[name]

    def materialize(self):
        """cut this split's tables out of the batch and let go of the batch"""
        for a in ('scaffold', 'covT', 'raw_snp_table', 'raw_linkage_table'):
            getattr(self, a)
        src = self.__dict__.get('_src')
        if src is not None and src[0].pileup_counts is not None:
            getattr(self, 'pileup_counts')
        if src is not None and src[0].ao is not None:
            getattr(self, 'read_to_snvs')
        self.__dict__.pop('_src', None)
        return self

    def __getstate__(self):
        # The reference puts split objects on multiprocessing queues (profile_controller.py:273-314): a pickled split
        # carries its OWN tables, not the arrays of the whole device batch it was cut from
        self.materialize()
        return dict(self.__dict__)

    def __setstate__(self, state):
        self.__dict__.update(state)

    # what the merge step copies from a split / from the ScaffoldSplitObject (profile_utilities.py:831-858)
    _OWN_FIELDS = ('scaffold', 'bam', 'length', 'raw_snp_table', 'raw_linkage_table', 'covT', 'clonT', 'clonTR', 'min_freq')
    _OPTIONAL_FIELDS = ('read_to_snvs', 'mm_to_position_graph', 'pileup_counts', 'profile_genes', 'gene_database', 'gene2sequence')
    _PARENT_FIELDS = ('profile_genes', 'gene_database', 'gene2sequence')

    def merge_single_profile(self, ScaffoldSplitObject, profile_class=None):
        """A scaffold of one split becomes its scaffold_profile (profile_utilities.py:831-858).  profile_class: the class to
        instantiate -- inside the reference's process the caller passes inStrain's own scaffold_profile (what its merge
        worker and everything downstream expect); default: the mirror below."""
        Sprofile = (profile_class or SCAFFOLD_PROFILE_CLASS or scaffold_profile)()
        for att in SplitObject._OWN_FIELDS:
            setattr(Sprofile, att, getattr(self, att))
        Sprofile.null_model = ScaffoldSplitObject.null_model
        for att in SplitObject._OPTIONAL_FIELDS:
            if att in self.__dict__ or (att in ('pileup_counts', 'read_to_snvs', 'mm_to_position_graph') and hasattr(self, att)):
                setattr(Sprofile, att, getattr(self, att))
        for att in SplitObject._PARENT_FIELDS:
            if hasattr(ScaffoldSplitObject, att):
                setattr(Sprofile, att, getattr(ScaffoldSplitObject, att))
        Sprofile.make_cumulative_tables()
        return Sprofile


# The class SplitObject.merge_single_profile instantiates when the caller names none.  The reference's merge worker calls
# split.merge_single_profile(self) with one argument and expects ITS scaffold_profile back: an integration sets this once
# (instrain_amd.profile.profile_utilities.SCAFFOLD_PROFILE_CLASS = inStrain...scaffold_profile); product
# code never imports the reference itself.
SCAFFOLD_PROFILE_CLASS = None


def merge_basewise(mm2array_list):
    """profile_utilities.py:408-419"""
    mms = set()
    for d in mm2array_list:
        mms |= set(d.keys())
    return {mm: pd.concat([d[mm] for d in mm2array_list if mm in d], verify_integrity=True) for mm in mms}


class scaffold_profile():
    '''Profile of a single scaffold (profile_utilities.py:860-896): what ScaffoldSplitObject.merge assembles'''

    def __init__(self, **kwargs):
        self.version = "instrain_amd"

    @classmethod
    def from_splits(cls, splits, null_model=None):
        """ScaffoldSplitObject.merge (profile_utilities.py:752-814) for an ordered list of SplitObjects"""
        if len(splits) == 1:
            class _Holder:
                pass
            h = _Holder()
            h.null_model = null_model
            P = cls()
            S = splits[0]
            for att in ['scaffold', 'bam', 'length', 'raw_snp_table', 'raw_linkage_table', 'covT', 'clonT', 'clonTR', 'min_freq']:
                setattr(P, att, getattr(S, att))
            P.null_model = null_model
            P.make_cumulative_tables()
            return P
        P = cls()
        P.null_model = null_model
        for att in ['scaffold', 'bam', 'min_freq']:
            vals = set(getattr(S, att) for S in splits)
            assert len(vals) == 1, vals
            setattr(P, att, list(vals)[0])
        P.length = sum(S.length for S in splits)
        for att in ['raw_snp_table', 'raw_linkage_table']:
            setattr(P, att, pd.concat([getattr(S, att) for S in splits]).reset_index(drop=True))
        for att in ['covT', 'clonT', 'clonTR']:
            setattr(P, att, merge_basewise([getattr(S, att) for S in splits]))
        P.make_cumulative_tables()
        return P

    def make_cumulative_tables(self):
        if self.raw_snp_table is not None:
            self.cumulative_snv_table = _parse_Sdb(_make_snp_table(self.raw_snp_table))
        self.cumulative_scaffold_table = make_coverage_table_host(self.covT, self.clonT, self.clonTR, self.length,
                                                                  self.scaffold, self.raw_snp_table)


def _make_snp_table(Stable):
    """profile_utilities.py:576-596: the raw table with its two string columns as categories; no rows / no table -> empty"""
    if Stable is False or Stable is None or 'scaffold' not in getattr(Stable, 'columns', ()):
        return pd.DataFrame()
    return pd.DataFrame(Stable).astype({'scaffold': 'category', 'con_base': 'category'})


def _parse_Sdb(sdb):
    """profile_utilities.py:598-612: var_freq / con_freq / ref_freq (count of the base / position_coverage)"""
    if len(sdb) == 0:
        return sdb
    cnt = np.stack([sdb[b].values.astype(np.float64) for b in "ACTG"], axis=1)
    cov = sdb['position_coverage'].values.astype(np.float64)
    col = {b: i for i, b in enumerate("ACTG")}
    rows = np.arange(len(sdb))
    for out, src in (('var_freq', 'var_base'), ('con_freq', 'con_base')):
        idx = np.array([col[v] for v in sdb[src].values])
        sdb[out] = cnt[rows, idx] / cov
    ref = sdb['ref_base'].values
    ok = np.array([v in col for v in ref])
    idx = np.array([col.get(v, 0) for v in ref])
    sdb['ref_freq'] = np.where(ok, cnt[rows, idx] / cov, np.nan)
    return sdb


def estimate_breadth(coverage):
    """profile_utilities.py:548-555"""
    return (-1) * np.exp(-1 * ((0.883) * coverage)) + 1


def calc_snps(Odb, mm):
    """snv_utilities.py:249-272 on a raw_snp_table: numpy pass (highest mm <= mm per position)"""
    if len(Odb) == 0:
        return [0, 0, 0, 0, 0]
    m = Odb['mm'].values
    k = m <= mm
    if not k.any():
        return [0, 0, 0, 0, 0]
    pos, mmv = Odb['position'].values[k], m[k]
    ac, cls = Odb['allele_count'].values[k], Odb['class'].values[k]
    order = np.lexsort((mmv, pos))
    last = np.r_[pos[order][1:] != pos[order][:-1], True]          # last (highest-mm) row of every position
    sel = order[last]
    ac, cls = ac[sel], cls[sel]
    con = np.isin(cls, ['SNS', 'con_SNV', 'pop_SNV'])
    pop = np.isin(cls, ['SNS', 'pop_SNV'])
    return [int((ac == 1).sum()), int((ac > 1).sum()), int(len(sel)), int(con.sum()), int(pop.sum())]


def make_coverage_table_host(covT, clonT, clonTR, lengt, scaff, SNPTable):
    """make_coverage_table (profile_utilities.py:425-506) from the shrunk per-mm Series, in numpy: one row per mm key
    of covT; coverage cumulated over levels <= mm, clonalities of the highest level <= mm per position."""
    table = {k: [] for k in COVERAGE_COLUMNS}
    lengt = int(lengt)
    cov = np.zeros(lengt, dtype=np.float64)
    cl = {}
    clr = {}
    snp = SNPTable if SNPTable is not None else pd.DataFrame()
    done = set()
    for mm in sorted(covT.keys()):
        for m2 in sorted(k for k in covT.keys() if k <= mm and k not in done):
            ser = covT[m2]
            cov[ser.index.values] += ser.values
            done.add(m2)
        for src, dst in ((clonT, cl), (clonTR, clr)):
            for m2 in sorted(int(k) for k in src.keys() if int(k) <= int(mm) and ('d', int(k), id(src)) not in done):
                dst.update(src[m2].to_dict())
                done.add(('d', m2, id(src)))
        clons = list(cl.values())
        Rclons = list(clr.values())
        counted, rare = len(clons), len(Rclons)
        SNS_count, SNV_count, div_site_count, con_snps, pop_snps = calc_snps(snp, mm)
        table['scaffold'].append(scaff)
        table['length'].append(lengt)
        table['breadth'].append(np.count_nonzero(cov) / lengt)
        table['coverage'].append(np.mean(cov))
        table['coverage_median'].append(int(np.median(cov)))
        table['coverage_std'].append(np.std(cov))
        table['coverage_SEM'].append(np.std(cov, ddof=1) / np.sqrt(lengt) if lengt > 1 else np.nan)
        for vals, a, b in ((clons, 'nucl_diversity', 'nucl_diversity_median'),
                           (Rclons, 'nucl_diversity_rarefied', 'nucl_diversity_rarefied_median')):
            if len(vals) > 0:
                table[a].append(1 - np.mean(vals))
                table[b].append(1 - np.median(vals))
            else:
                table[a].append(np.nan)
                table[b].append(np.nan)
        table['breadth_minCov'].append(counted / lengt)
        table['breadth_rarefied'].append(rare / lengt)
        table['breadth_expected'].append(estimate_breadth(table['coverage'][-1]))
        table['divergent_site_count'].append(div_site_count)
        table['SNS_count'].append(SNS_count)
        table['SNV_count'].append(SNV_count)
        table['consensus_divergent_sites'].append(con_snps)
        table['population_divergent_sites'].append(pop_snps)
        table['conANI_reference'].append((counted - con_snps) / counted if counted else 0)
        table['popANI_reference'].append((counted - pop_snps) / counted if counted else 0)
        table['mm'].append(mm)
    return pd.DataFrame(table, columns=COVERAGE_COLUMNS)


def make_coverage_table(levels, lengt, scaff, SNPTable, snv_counts=None):
    """Mirror of make_coverage_table (profile_utilities.py:425-506): `levels` = this scaffold's row of
    Batch.summarize() (device aggregates per mm); the SNV-table columns are computed here from SNPTable -- or taken from
    snv_counts, the scaffold's row of engine.snv_level_counts (one SNV_LEVEL_DT record per level of `levels`)."""
    table = {k: [] for k in COVERAGE_COLUMNS}
    n = float(lengt)
    for j, r in enumerate(levels):
        if not r['present']:
            continue                                    # not a key of covT for this scaffold
        mm = int(r['mm'])
        s1, s2 = float(r['sum_cov']), float(r['sumsq_cov'])
        mean = s1 / n
        var = max(s2 / n - mean * mean, 0.0)
        counted, rare = int(r['counted']), int(r['counted_rarefied'])
        if snv_counts is None:
            SNS_count, SNV_count, div_site_count, con_snps, pop_snps = calc_snps(SNPTable, mm)
        else:
            SNS_count, SNV_count, div_site_count, con_snps, pop_snps = (int(snv_counts[j][f]) for f in ('sns', 'snv', 'divergent', 'con', 'pop'))
        table['scaffold'].append(scaff)
        table['length'].append(lengt)
        table['breadth'].append(int(r['nonzero']) / lengt)
        table['coverage'].append(mean)
        table['coverage_median'].append(int(r['median_cov']))
        table['coverage_std'].append(np.sqrt(var))
        table['coverage_SEM'].append(np.sqrt(var * n / (n - 1)) / np.sqrt(n) if lengt > 1 else np.nan)
        table['nucl_diversity'].append(1 - r['sum_clon'] / counted if counted else np.nan)
        table['nucl_diversity_median'].append(1 - r['median_clon'] if counted else np.nan)
        table['nucl_diversity_rarefied'].append(1 - r['sum_clon_rarefied'] / rare if rare else np.nan)
        table['nucl_diversity_rarefied_median'].append(1 - r['median_clon_rarefied'] if rare else np.nan)
        table['breadth_minCov'].append(counted / lengt)
        table['breadth_rarefied'].append(rare / lengt)
        table['breadth_expected'].append(estimate_breadth(mean))
        table['divergent_site_count'].append(div_site_count)
        table['SNS_count'].append(SNS_count)
        table['SNV_count'].append(SNV_count)
        table['consensus_divergent_sites'].append(con_snps)
        table['population_divergent_sites'].append(pop_snps)
        table['conANI_reference'].append((counted - con_snps) / counted if counted else 0)
        table['popANI_reference'].append((counted - pop_snps) / counted if counted else 0)
        table['mm'].append(mm)
    return pd.DataFrame(table, columns=COVERAGE_COLUMNS)


def get_worker_log(worker_type, unit, status, when=None, mem=None):
    """logUtils.get_worker_log (logUtils.py:939-975): "\nWorkerLog worker_type unit status RAM time PID" -- the line
    profile_controller.py:288-289 collects from SplitObject.log and the log parser reads (linewords[0..6]).  `when`: the time
    stamp to report (a device batch profiles all its splits at once: they share the batch's start / end)."""
    assert status in ['start', 'end'], status
    if mem is None:
        mem = _rss()
    return "\nWorkerLog {0} {1} {2} {3} {4} {5}".format(worker_type, unit, status, mem, time.time() if when is None else when, os.getpid())


def _rss():
    try:
        import psutil
        return psutil.Process(os.getpid()).memory_info().rss
    except Exception:
        try:
            return int(open("/proc/self/statm").read().split()[1]) * os.sysconf("SC_PAGE_SIZE")
        except Exception:
            return 0


def tables_to_splits(res, split_bounds, split_scaffold, split_number, scaffold_offset, split_seq_len, min_freq,
                     bam_name=None, min_cov=5, started=None, mm_clamped=None, mm_values=None):
    """Batch result (engine.Batch.fetch() / Pipe.collect()) -> list of SplitObject, one per split, in split order.
    started: time.time() when the batch's profiling began (the start stamp of every split's worker log)."""
    tables = _BatchTables(res, split_bounds, split_scaffold, scaffold_offset, min_cov, mm_values=mm_values)
    t_end, mem = time.time(), _rss()
    tables.meta = {'scaffold': split_scaffold, 'number': split_number, 'length': split_seq_len, 'bam': bam_name, 'min_freq': min_freq,
                   't_start': t_end if started is None else started, 't_end': t_end, 'mem': mem, 'mm_clamped': mm_clamped}
    return [SplitObject._of_batch(tables, i) for i in range(len(split_bounds) - 1)]


def profile_splits(ctx, scaffolds, sequences, obs, pair, null_model, n_mm_bins, window_length=10000, bam_name=None,
                   **kwargs):
    """Profile every split of `scaffolds` in ONE device batch.

    scaffolds / sequences: names and upper-cased sequences laid end to end in the flat space (in the
    order the observations' gpos assume); obs / pair: packed observations (engine.OBS_DT) and pair ids.
    kwargs as the reference's profile_split: min_cov, min_freq, min_snp, rarefied_coverage.
    Returns {"{scaffold}.{split}": SplitObject} like Sprofile_dict (profile_utilities.py:85).
    """
    min_cov = int(kwargs.get('min_cov', 5))
    min_freq = float(kwargs.get('min_freq', .05))
    min_snp = int(kwargs.get('min_snp', 10))
    lut, fb = null_model_lut(null_model)
    ctx.set_null_model(lut, fb)
    bounds, s_scaff, s_num, s_off, s_len, _ = split_table(
        (name, len(seq), [(i, s, e) for i, (s, e) in enumerate(iterate_splits(len(seq), window_length))])
        for name, seq in zip(scaffolds, sequences))
    ref = np.concatenate([engine.encode_seq(s) for s in sequences])
    b = engine.Batch(ctx, ref, bounds, obs, pair, min_cov=min_cov, min_freq=min_freq, min_snp=min_snp,
                     rarefied_coverage=int(kwargs.get('rarefied_coverage', 5)), n_mm_bins=n_mm_bins,
                     enable_linkage=True, seed=int(kwargs.get('seed', 0)))
    t_started = time.time()
    try:
        b.run()
        res = b.fetch()
        if kwargs.get('store_everything'):          # read_to_snvs / mm_to_position_graph are made from these (profile/linkage.py)
            res["allele_obs"] = b.fetch_allele_obs()
            res["pair_names"] = kwargs.get('pair_names')
        levels = None
        if kwargs.get('scaffold_tables') is not None:   # only the merge step's cumulative tables need the device summaries
            scaff_bounds = np.r_[0, np.cumsum([len(q) for q in sequences])]
            levels, _ = b.summarize(scaff_bounds)
    finally:
        b.close()
    splits = tables_to_splits(res, np.asarray(bounds), s_scaff, s_num, s_off, s_len, min_freq, bam_name, started=t_started)
    out = {"{0}.{1}".format(S.scaffold, S.split_number): S for S in splits}
    if kwargs.get('scaffold_tables') is not None:       # cumulative_scaffold_table per scaffold (merge step)
        for i, name in enumerate(scaffolds):
            snp = [S.raw_snp_table for S in splits if S.scaffold == name and len(S.raw_snp_table)]
            snp = pd.concat(snp) if snp else pd.DataFrame()
            kwargs['scaffold_tables'][name] = make_coverage_table(levels[i], len(sequences[i]), name, snp)
    return out


def _failure_log(scaffold, split_number):
    t = time.strftime('%m-%d %H:%M')
    return "\n{1} DEBUG FAILURE SplitException {0} {2}\n".format(scaffold, t, split_number)   # profile_utilities.py:108-110


def _fail(logs, scaffold, split_numbers, exc=None):
    """a scaffold that is dropped: its exception on stdout, the reference's line for every one of its splits"""
    if exc is not None:
        print(exc)
        traceback.print_exc()
    for n in split_numbers:
        line = _failure_log(scaffold, n)
        logging.error(line)
        if logs is not None:
            logs.append(line)


def plan_scaffolds(fasta_db, wanted_lengths, window_length):
    """{scaffold: [(split_number, start, end), ...]} for every scaffold of `wanted_lengths` (name -> length), and
    {scaffold: exception} for those whose splits are unusable.  With a fasta_db its rows decide (fasta.py:33-40,
    profile_controller.py:415-433) -- ONE pass over the table (factorize + one sort), like the reference's single groupby
    (:420), not one filter of the whole table per scaffold; without it iterate_splits (fasta.py:56-73).
    _validate_splits (fasta.py:75-85): 0-based, double inclusive, tiling the scaffold."""
    plan, bad = {}, {}
    if fasta_db is None:
        for name, ln in wanted_lengths.items():
            plan[name] = [(i, s, e) for i, (s, e) in enumerate(iterate_splits(ln, window_length))]
        return plan, bad
    codes, names = pd.factorize(fasta_db['scaffold'].values, sort=False)
    start = fasta_db['start'].values.astype(np.int64)
    end = fasta_db['end'].values.astype(np.int64)
    num = fasta_db['split_number'].values.astype(np.int64)
    order = np.lexsort((start, codes))
    codes_o, start_o, end_o, num_o = codes[order], start[order], end[order], num[order]
    first = np.r_[0, np.flatnonzero(np.diff(codes_o)) + 1, len(codes_o)] if len(codes_o) else np.zeros(1, np.int64)
    tiles = np.ones(len(codes_o), dtype=bool)
    if len(codes_o) > 1:
        tiles[1:] = (end_o[:-1] + 1 == start_o[1:]) | (codes_o[1:] != codes_o[:-1])
    bad_rows = np.add.reduceat(~tiles, first[:-1]) if len(codes_o) else np.zeros(0, np.int64)
    for g in range(len(first) - 1):
        a, e = int(first[g]), int(first[g + 1])
        name = names[codes_o[a]]
        if name not in wanted_lengths:
            continue
        ln = wanted_lengths[name]
        if start_o[a] != 0 or end_o[e - 1] != ln - 1 or bad_rows[g]:
            bad[name] = ValueError("fasta_db splits of {0} do not tile [0, {1})".format(name, ln))
            continue
        plan[name] = list(zip(num_o[a:e].tolist(), start_o[a:e].tolist(), end_o[a:e].tolist()))
    return plan, bad


def split_table(scaffolds):
    """(name, length, [(split_number, start, end), ...]) of scaffolds laid end to end -> the flat split table of their batch: bounds (every
    split's first flat position + the total length), per split its scaffold / number / scaffold offset / length, and first_split (every
    scaffold's first row + the row count)"""
    bounds, s_scaff, s_num, s_off, s_len, first_split = [], [], [], [], [], []
    off = 0
    for name, length, splits in scaffolds:
        first_split.append(len(bounds))
        for num, s, e in splits:
            bounds.append(off + s)
            s_scaff.append(name); s_num.append(num); s_off.append(off); s_len.append(e - s + 1)
        off += length
    first_split.append(len(bounds))
    bounds.append(off)
    return bounds, s_scaff, s_num, s_off, s_len, first_split


def read_filter_flags(kwargs):
    """the read filter's flags with the CLI's defaults (filter_reads.py): what BamFile.filter and the expansion take"""
    return dict(min_read_ani=kwargs.get('min_read_ani', 0.95), min_mapq=kwargs.get('min_mapq', -1),
                max_insert_relative=kwargs.get('max_insert_relative', 3), min_insert=kwargs.get('min_insert', 50),
                pairing_filter=kwargs.get('pairing_filter', 'paired_only'))


def profile_options(kwargs):
    """profile_bam's kwargs parsed once: every default of the run is here and nowhere else.  pipe_depth / layout / jump_slack stay None
    unless the caller names them: their defaults follow from the run (number of batches, mm levels; pipe_depth_of, open_pipe)."""
    o = types.SimpleNamespace()
    o.window_length = int(kwargs.get('window_length', 10000))
    o.skip_mm = bool(kwargs.get('skip_mm_profiling', False))
    o.min_cov = int(kwargs.get('min_cov', 5))
    o.min_freq = float(kwargs.get('min_freq', .05))
    o.min_snp = int(kwargs.get('min_snp', 10))
    # the CLI always passes its own default of 50 (argumentParser.py:170); profile_split's fallback of 5 (:143) is never reached from it
    o.rarefied = int(kwargs.get('rarefied_coverage', 50))
    o.seed = int(kwargs.get('seed', 0))
    o.store_everything = bool(kwargs.get('store_everything', False))
    o.strict = bool(kwargs.get('strict'))
    o.device = int(kwargs.get('device', 0))
    o.host_threads = int(kwargs.get('host_threads', 0))
    # pass 1 (inflate + record walk) may run on another number of threads than the hand-over
    # (2 x host_threads measured both ways box to box in round 6: 180 -> 137 ms once, 155 -> 180 ms another time; the caller may choose)
    o.scan_threads = int(kwargs.get('scan_threads', o.host_threads))
    o.batch_positions = int(kwargs.get('batch_positions', 64_000_000))
    if 'batch_reads' in kwargs:
        o.batch_segs = int(kwargs['batch_reads'])
    else:
        o.batch_segs = max(64, int(kwargs['batch_observations']) // 150) if 'batch_observations' in kwargs else 4_000_000
    o.pipe_depth, o.layout, o.jump_slack = kwargs.get('pipe_depth'), kwargs.get('layout'), kwargs.get('jump_slack')
    o.filter = read_filter_flags(kwargs)
    # what only a caller that shares the file's scan hands over (dist.profile_bam_sharded)
    o.scan_part, o.median_insert, o.filter_refs = kwargs.get('scan_part'), kwargs.get('median_insert'), kwargs.get('filter_refs')
    o.priority_reads = kwargs.get('priority_reads')
    # the filters that read the read report (profile/fasta.py:87-136); --database_mode is three other flags (controller.py:210-214)
    o.min_scaffold_reads = kwargs.get('min_scaffold_reads', 0) or 0
    o.min_genome_coverage = kwargs.get('min_genome_coverage', 0) or 0
    if kwargs.get('database_mode'):
        o.filter['min_read_ani'] = 0.92
        o.skip_mm = True
        o.min_genome_coverage = 1
    o.read_tables = kwargs.get('read_tables')
    # (mapping_info, {removed scaffold: reason}) of the WHOLE file from a caller that shares the scan (dist.profile_bam_sharded): its handle
    # has then run the final filter and dropped the removed scaffolds already -- neither happens again here
    o.read_report_done = kwargs.get('read_report_done')
    return o


def select_scaffolds(refs, s2s, fasta_db, window_length, bam):
    """Which scaffolds can be profiled at all.  refs: the BAM header's (name, length, ...) rows; fasta_db decides which are wanted
    (without it every reference that has a sequence).  -> plan = [(tid, name, [(split_number, start, end), ...])] in file order (the
    stream stays position-clustered), failed = {name: (exception, number of failure lines)}"""
    tid_of = {n: i for i, (n, _, _) in enumerate(refs)}
    if fasta_db is not None:
        wanted = list(dict.fromkeys(fasta_db['scaffold'].values.tolist()))
        rows_of = fasta_db['scaffold'].value_counts(sort=False).to_dict()
    else:
        wanted = [n for n, _, _ in refs if n in s2s]
        rows_of = {}
    usable, failed = {}, {}
    for name in wanted:
        if name not in tid_of:                   # samfile.pileup raises ValueError -> (None, log) (profile_utilities.py:154-156)
            failed[name] = ValueError("scaffold {0} is not in the .bam file {1}!".format(name, bam))
        elif name not in s2s or len(s2s[name]) != refs[tid_of[name]][1]:
            failed[name] = ValueError("scaffold {0} has no sequence / its length differs from the .bam header".format(name))
        else:
            usable[name] = refs[tid_of[name]][1]
    splits_of, bad = plan_scaffolds(fasta_db, usable, window_length)
    failed.update(bad)
    plan = sorted((tid_of[name], name, sp) for name, sp in splits_of.items())
    return plan, {name: (e, int(rows_of.get(name, 1))) for name, e in failed.items()}


def choose_read_pairs(bf, plan, n_refs, sR2M, opt):
    """Which read pairs of the scanned file count, and with which mm: the controller's R2M, or the built-in filter (-> the reference
    indices that existed for it)"""
    if sR2M is None:
        if opt.priority_reads:
            bf.set_priority_reads(opt.priority_reads)
        # the reference's filter only ever sees the scaffolds of the fasta (filter_reads.py:63-77): a BAM mapped to a larger
        # database must not let the other references into the median insert / the cross-scaffold look-ups
        wanted_tids = opt.filter_refs
        if wanted_tids is None:
            wanted_tids = [t for t, _, _ in plan] if len(plan) < n_refs else []
        if opt.read_report_done is None:            # (else the caller's handle is filtered, on the same set)
            bf.set_wanted_refs(wanted_tids)
            bf.filter(median_insert=opt.median_insert, **opt.filter)
        return list(wanted_tids) if len(wanted_tids) else list(range(n_refs))
    for tid, name, _ in plan:
        r2m = sR2M.get(name, {})
        if isinstance(r2m, (set, frozenset, list, tuple)):       # --skip_mm_profiling: a set of pair names
            bf.set_r2m(tid, list(r2m), None)
        else:
            bf.set_r2m(tid, list(r2m.keys()), [0 if opt.skip_mm else int(v) for v in r2m.values()])
    bf.scan(part=opt.scan_part)                  # refresh the totals (max_mm now comes from the controller's values)


def read_report_step(bf, plan, refs, wanted_tids, opt, stb):
    """The read report of the filter that just ran and the scaffold filters that read it (controller.py:260-272): -> (mapping_info
    over all wanted scaffolds, made before anything is dropped; {removed scaffold: reason}; the plan's rows that stay, still in
    file order -- the reference sorts the survivors by read count, which no table depends on).  The handle forgets the removed
    scaffolds' pairs (BamFile.drop_refs): the mm levels, the segment estimate and the batches then see only what will be profiled."""
    names = [n for n, _, _ in refs]
    if opt.read_report_done is not None:
        rdb, removed = opt.read_report_done
        return rdb, removed, [k for k, (_, name, _) in enumerate(plan) if name not in removed]
    rdb = filter_reads.mapping_info(bf.read_report(), names, wanted_tids)
    removed = {}
    if opt.min_scaffold_reads or opt.min_genome_coverage:
        s2p = rdb.set_index('scaffold')['filtered_pairs'].to_dict()
        wanted = [names[t] for t in sorted(wanted_tids)]
        _, removed = filter_reads.filter_scaffolds(wanted, s2p, {n: ln for n, ln, _ in refs}, float(rdb.loc[0, 'mean_pair_length']),
                                                   min_scaffold_reads=opt.min_scaffold_reads, min_genome_coverage=opt.min_genome_coverage,
                                                   stb=stb)
        if removed:
            tid_of = {n: t for t, n in enumerate(names)}
            bf.drop_refs([tid_of[n] for n in removed])
    keep = [k for k, (_, name, _) in enumerate(plan) if name not in removed]
    return rdb, removed, keep


def mm_levels(bf, skip_mm, strict):
    """The mm levels the kept pairs travel with -> n_mm (bins of a device batch), mm_values (None, or rank -> the pairs' mm), mm_clamped
    (None, or the mm the pairs beyond the 128th level are counted at)"""
    n_mm = 1 if skip_mm else int(bf.info["max_mm"]) + 1
    mm_clamped = None
    mm_values = None
    bf.set_mm_levels([])
    bf.set_mm_cap(0x7FFFFFFF)
    if n_mm > 128:
        # the reference bins any mm (profile_utilities.py:268-286); a device batch indexes 128 levels.  Every table depends on the
        # ORDER of the levels alone (counts are cumulated over the levels <= mm, :297-312), so the pairs travel with the RANK of
        # their mm among the values that occur and the tables' levels are mapped back (round 6: exact for any mm as long as no
        # more than 128 DIFFERENT values occur among the kept pairs)
        mm_values = np.asarray(bf.mm_levels(), dtype=np.int64)
        bf.set_mm_levels(mm_values)
        n_mm = len(mm_values)
        if n_mm > 128:
            # more than 128 different values: the pairs beyond the 128th are piled up AT it (their bases then appear early in the
            # cumulative tables of the levels from there on) -- loudly, on every SplitObject (S.mm_clamped = that value), and never
            # under strict=True: a caller that asked for exactness gets the error instead of merged levels
            if strict:
                raise ValueError("read pairs with {0} different numbers of mismatches (up to {1}): the device bins 128 mm levels "
                                 "(strict=True refuses to merge the levels beyond; --skip_mm_profiling or a higher --min_read_ani "
                                 "avoids this)".format(n_mm, int(mm_values[-1])))
            mm_clamped = int(mm_values[127])
            logging.warning("read pairs with {0} different numbers of mismatches: the device bins 128 mm levels, pairs beyond {1} "
                            "mismatches are counted at that level (--skip_mm_profiling or a higher --min_read_ani avoids "
                            "this)".format(n_mm, mm_clamped))
            bf.set_mm_cap(127)
            mm_values = mm_values[:128]
            n_mm = 128
    return n_mm, mm_values, mm_clamped


def estimate_segments(info, reads_per_ref, plan):
    """Read segments every scaffold of the plan will be: a read = one segment per 150 aligned columns (2 x 250 / 2 x 300 libraries: two
    or more) + one per indel; the mean read length comes from the filter's tallies in `info` (sum of the kept pairs' query lengths,
    controller.py:309-310)"""
    fp, fb = int(info.get("filtered_pairs", 0) or 0), int(info.get("filtered_bases", 0) or 0)
    mean_len = fb / (2.0 * fp) if fp > 0 and fb > 0 else 150.0
    per_read = float(-(-int(np.ceil(mean_len)) // 150)) + 0.25
    return [int(reads_per_ref[tid] * per_read) + 64 for tid, _, _ in plan]


def largest_need(item_groups, plan, refs, est_segs):
    """(positions, segments, splits) a pipe must hold for the largest group: it follows from the plan alone"""
    return (max(sum(refs[plan[k][0]][1] for k in items) for items in item_groups),
            max(sum(est_segs[k] for k in items) for items in item_groups),
            max(sum(len(plan[k][2]) for k in items) + 1 for items in item_groups))


def pipe_depth_of(opt, n_groups):
    """device batches in flight"""
    return max(1, int((2 if n_groups > 1 else 1) if opt.pipe_depth is None else opt.pipe_depth))


def open_pipe(ctx, opt, n_mm, depth, need, pool=False):
    """The read-level pipe of a run for batches of up to `need` = (positions, segments, splits); pipe.cap = what it was made with.
    pool: the run's slots are pulled for SNV pooling (SampleSet.pool_add), which reads a one-level slot's count table"""
    cap = (max(need[0], 1 << 16), max(need[1], 1 << 12), max(need[2], 64))
    pp = engine.Pipe(ctx, max_pos=cap[0], max_obs=0, max_segs=cap[1], max_splits=cap[2], depth=depth,
                     host_threads=opt.host_threads, pin_threads=False,
                     min_cov=opt.min_cov, min_freq=opt.min_freq, min_snp=opt.min_snp,
                     rarefied_coverage=opt.rarefied, n_mm_bins=n_mm,
                     enable_linkage=True, seed=opt.seed, want_counts=opt.store_everything or (pool and n_mm == 1),
                     # mm profiling on: the front end emits bit planes + the pairs' levels, the batches travel as 32-byte
                     # reference-delta records with the level in the header (round 6) -- half the bytes, the 14-ns stager
                     layout=int((_lib.LAYOUT_MM_DELTA_RECORDS if n_mm > 1 else 0) if opt.layout is None else opt.layout),
                     # (a read that differs from the reference at more than three columns is several delta records: pairs kept at
                     # 95 % identity carry up to 15 mismatches -- room for their pieces)
                     jump_slack=float((1.0 if n_mm > 1 else 0.0) if opt.jump_slack is None else opt.jump_slack))
    pp.cap = cap
    return pp


def _encode_scaffold(seq):
    return engine.encode_seq(str(seq).upper())


class _StageClock:
    """stats[name] += the milliseconds since the last stamp (profile_bam's `stats`; nothing without one)"""

    def __init__(self, stats):
        self.stats, self.t = stats, time.perf_counter()

    def __call__(self, name):
        if self.stats is not None:
            now = time.perf_counter()
            self.stats[name] = self.stats.get(name, 0.0) + (now - self.t) * 1e3
            self.t = now


class _Group:
    """one device batch of whole scaffolds: its flat layout"""
    __slots__ = ("items", "tids", "bounds", "s_scaff", "s_num", "s_off", "s_len", "ref", "n_pos", "first_split", "ticket", "est_segs", "t_submit", "pair_names")


class _BatchRun:
    """profile_bam's batch loop: groups of whole scaffolds go through a pipe, at most `depth` in flight, collected in submission order
    into `out`.  A group the pipe is too small for gets a larger pipe (grow_and_submit); a group whose batch fails is profiled scaffold by
    scaffold so that only the offender is dropped (run_alone).  The pipe comes from `make_pipe(need)`; every ticket is collected and
    released on the pipe that issued it -- the pipe is only replaced while nothing is in flight."""

    def __init__(self, bf, plan, refs, opt, make_pipe, depth, codes_of, est_segs, out, stage, bam=None, mm_values=None, mm_clamped=None,
                 gset=None, logs=None, scaffold_tables=None, scaffold_levels=None, genomes=None, compare_set=None, compare_sample=None,
                 irep=None, irep_index=None, pool_set=None, pool_sample=None):
        self.bf, self.plan, self.refs, self.opt, self.make_pipe, self.depth = bf, plan, refs, opt, make_pipe, depth
        self.codes_of, self.est_segs, self.out, self.stage, self.bam = codes_of, est_segs, out, stage, bam
        self.mm_values, self.mm_clamped, self.gset, self.logs = mm_values, mm_clamped, gset, logs
        self.scaffold_tables, self.scaffold_levels = scaffold_tables, scaffold_levels
        self.genomes = genomes                       # genome_utilities.GenomeTables (profile_bam(stb=...)) or None
        self.compare_set, self.compare_sample = compare_set, compare_sample    # compare.SampleSet that gets every batch's sketch, or None
        self.pool_set, self.pool_sample = pool_set, pool_sample    # compare.SampleSet (after pool_sites()) that pulls every batch's counts, or None
        self.irep, self.irep_index = irep, irep_index or {}    # engine.IRep of the run's genomes (scaffold name -> its index there), or None
        self.ekw = dict(opt.filter, skip_mm=opt.skip_mm, window_length=opt.window_length)
        self.pipe = self.cap = None
        self.in_flight = []                          # submitted, not yet collected (at most `depth`)

    def open_pipe(self, need):
        self.pipe = self.make_pipe(need)
        self.cap = need

    def layout(self, items):
        g = _Group()
        g.items, g.tids = items, [self.plan[k][0] for k in items]
        bounds, g.s_scaff, g.s_num, g.s_off, g.s_len, g.first_split = split_table(
            (self.plan[k][1], self.refs[self.plan[k][0]][1], self.plan[k][2]) for k in items)
        seqs = [self.codes_of[k].result() for k in items]
        g.bounds = np.asarray(bounds, np.int64)
        g.ref = np.concatenate(seqs) if len(seqs) > 1 else seqs[0]
        g.n_pos = bounds[-1]
        g.est_segs = sum(self.est_segs[k] for k in items)
        g.ticket = g.t_submit = g.pair_names = None
        return g

    def submit(self, g):
        """the front end's pass 2 for the group's scaffolds + hand-over; returns False when the pipe is too small"""
        try:
            g.ticket = self.pipe.submit_bam(self.bf, g.tids, g.ref, g.bounds, **self.ekw)
            g.t_submit = time.time()
            if self.opt.store_everything:
                g.pair_names = self.bf.batch_pair_names()
            return True
        except engine.IsxError as e:
            if e.code != _lib.ERR_CAPACITY:
                raise
            if os.environ.get("ISX_PROFILE_DEBUG"):
                print("submit_bam:", e)
            return False

    def grow_and_submit(self, g, floor, base):
        """The pipe was too small for g (the estimate was short: many indels / long reads, reads that are many records each), and nothing
        is in flight: up to three larger pipes, 2 / 8 / 32 x `base` segments -- always of the base, never of an already grown value -- and
        at least what the front end counted on the attempt before, nowhere below `floor` = (positions, segments, splits).  -> did it fit"""
        for factor in (2, 8, 32):
            n_real = int((self.bf.info or {}).get("n_segs", 0))
            need = (max(floor[0], g.n_pos), max(factor * base, n_real + 4096), max(floor[2], len(g.bounds)))
            self.pipe.close()
            self.open_pipe(need)
            if self.submit(g):
                return True
        return False

    def collect(self, g):
        """tables of a submitted group -> SplitObjects"""
        t, opt = g.ticket, self.opt
        try:
            res = self.pipe.collect(t, rare_list=False, densify=False, shrunk_entries=not opt.store_everything)
            self.stage("collect_wait_ms")
            if "_result" in res:                    # mm profiling on: own copies of the level-sparse tables (1-3 bytes a level); the columns the
                res["level_tables"] = self.pipe.levels_copy(res)     # splits' covT / clonT / clonTR are cut from are made on first access
            if opt.store_everything:                # read_to_snvs / mm_to_position_graph of the splits are made from these
                res["allele_obs"] = res["slot"].fetch_allele_obs()
                res["pair_names"] = g.pair_names
            splits = tables_to_splits(res, g.bounds, g.s_scaff, g.s_num, g.s_off, g.s_len, opt.min_freq, self.bam,
                                      min_cov=opt.min_cov, started=g.t_submit, mm_clamped=self.mm_clamped, mm_values=self.mm_values)
            summaries = self.scaffold_tables is not None or self.scaffold_levels is not None or self.genomes is not None
            genes = self.gset is not None and bool(splits)
            if summaries or genes or self.compare_set is not None or self.pool_set is not None:
                sb = np.r_[0, np.cumsum([self.refs[tid][1] for tid in g.tids])]
                if summaries:
                    self.summarize(g, res["slot"], splits, sb)
                if genes:
                    self.profile_genes(g, res["slot"], splits, sb)
                if self.compare_set is not None:    # the slot's sketch (compare.SampleSet) before the slot goes back to the pipe
                    self.compare_set.add_batch(self.compare_sample, res["slot"], [self.plan[k][1] for k in g.items], sb, self.mm_values)
                if self.pool_set is not None:       # the second pass of SNV pooling: the slot's counts at the sites the sample does not own
                    self.pool_set.pool_add(self.pool_sample, res["slot"], [self.plan[k][1] for k in g.items], sb)
        finally:
            self.pipe.release(t)
            g.ticket = None
        return splits

    def summarize(self, g, slot, splits, sb):
        """scaffold_levels / scaffold_tables of the group's scaffolds from the device summaries"""
        levels, _ = slot.summarize(sb)
        if self.mm_values is not None:              # the device's levels are ranks: back to the pairs' mm
            for lv in levels:
                lv['mm'] = self.mm_values[lv['mm'].astype(np.int64)]
        tables = splits[0]._src[0] if splits else None
        snv_levels = None
        if self.genomes is not None:                # the batch's share of genome_info: everything below only ever adds
            snv_levels = self.roll_up_genomes(g, slot, tables, sb, levels)
        for j, k in enumerate(g.items):
            tid, name, _ = self.plan[k]
            if self.scaffold_levels is not None:    # the device's per-(scaffold, mm) aggregates as they are
                self.scaffold_levels[name] = levels[j][levels[j]['present'] != 0].copy()
            if self.scaffold_tables is not None:
                # the scaffold's rows in one cut -- not needed when the device counted them (calc_snps would be one lexsort per level)
                snp = tables.snp_table(g.first_split[j], g.first_split[j + 1]) if snv_levels is None else None
                self.scaffold_tables[name] = make_coverage_table(levels[j], self.refs[tid][1], name, snp,
                                                                 None if snv_levels is None else snv_levels[j])

    def roll_up_genomes(self, g, slot, tables, sb, levels):
        """SNV counts and linkage sums per (scaffold, level) and the genomes' coverage distribution of this batch, added to the
        run's GenomeTables -> the SNV counts [n_scaffolds, n_levels]"""
        names = [self.plan[k][1] for k in g.items]
        n_levels = slot.n_mm_bins
        empty = tables is None
        snv_levels, _ = engine.snv_level_counts(slot.ctx, np.zeros(0, _lib.SNV_DT) if empty else tables.snv, sb, n_levels)
        ld_levels, _ = engine.ld_level_sums(slot.ctx, np.zeros(0, _lib.LD_DT) if empty else tables.ld, sb, n_levels)
        ids, local = self.genomes.batch_genomes(names)
        acc = hist = None
        if local:
            acc, hist, _ = slot.genome_coverage(sb, ids, len(local), mask_edges=self.genomes.mask_edges)
        if self.irep is not None:                   # iRep's block sums: coverage up to mm == 1 (every level without mm profiling)
            self.irep.add(slot, sb, [self.irep_index.get(name, -1) for name in names],
                          self.genomes.irep_level(self.mm_values, n_levels, self.opt.skip_mm))
        self.genomes.add_batch(names, [self.refs[tid][1] for tid in g.tids], levels, snv_levels, ld_levels, local, acc, hist,
                               mms=self.mm_values)
        return snv_levels

    def profile_genes(self, g, slot, splits, sb):
        """profile_genes_from_profile of every scaffold of the batch (gene_profile.py)"""
        src = splits[0]._src[0]
        names = [self.plan[k][1] for k in g.items]
        snv = [_parse_Sdb(_make_snp_table(src.snp_table(g.first_split[j], g.first_split[j + 1]))) for j in range(len(names))]
        snv = [d for d in snv if len(d)]
        snv = pd.concat([d.astype({'scaffold': object, 'con_base': object}) for d in snv]) if snv else pd.DataFrame()
        gl = []
        gt = gene_profile.profile_batch(slot, self.gset, names, sb, snv, self.mm_values, gl)
        for line in gl:
            line = "\n{1} {0}".format(line, time.strftime('%m-%d %H:%M'))
            logging.error(line)
            if self.logs is not None:
                self.logs.append(line)
        for kk in gene_profile.TABLE_NAMES:
            self.gset.tables[kk].append(gt[kk])

    def take(self, splits):
        if not splits:
            return
        src = splits[0].__dict__.get('_src')
        if src is not None and all(S.__dict__.get('_src') is not None and S.__dict__['_src'][0] is src[0] for S in (splits[0], splits[-1])):
            m = src[0].meta                         # (the keys straight from the batch's split table: no per-object field is realised)
            self.out.update(zip(map("{0}.{1}".format, m['scaffold'], m['number']), splits))
        else:                                       # materialised / unpickled objects: their own fields
            self.out.update(("{0}.{1}".format(S.scaffold, S.split_number), S) for S in splits)

    def run_alone(self, items):
        """a group whose batch failed: scaffold by scaffold, so that only the offender is dropped (nothing is in flight)"""
        for k in items:
            try:
                g = self.layout([k])
                if not self.submit(g) and not self.grow_and_submit(g, (0, 0, 0), g.est_segs):
                    raise RuntimeError("scaffold does not fit a device batch")
                self.take(self.collect(g))
            except Exception as e2:
                _fail(self.logs, self.plan[k][1], [sp[0] for sp in self.plan[k][2]], e2)

    def drain_one(self):
        g = self.in_flight.pop(0)
        try:
            sp = self.collect(g)
            self.stage("collect_ms")
            self.take(sp)
        except Exception as e:
            print(e)
            traceback.print_exc()
            failed = [g]                            # run_alone may replace the pipe: bring every other batch home on this one first
            while self.in_flight:
                h = self.in_flight.pop(0)
                try:
                    self.take(self.collect(h))
                except Exception:
                    failed.append(h)
            for h in failed:
                self.run_alone(h.items)

    def drain(self):
        while self.in_flight:
            self.drain_one()

    def run(self, item_groups, layouts):
        """layouts[i]: the future of item_groups[i]'s _Group; dropped once used"""
        for gi, items in enumerate(item_groups):
            while len(self.in_flight) >= self.depth:
                self.drain_one()
            try:
                g = layouts[gi].result()
                layouts[gi] = None
                self.stage("layout_wait_ms")
                ok = self.submit(g)
                self.stage("submit_ms")
                if not ok:
                    self.drain()                    # a larger pipe once the batches in flight are home
                    if not self.grow_and_submit(g, self.cap, self.cap[1]):
                        raise RuntimeError("batch does not fit the device pipe")
                self.in_flight.append(g)
            except Exception as e:
                print(e)
                traceback.print_exc()
                self.drain()
                self.run_alone(items)
        self.drain()


def profile_bam(bam, fasta_db=None, sR2M=None, ISP_loc=None, **kwargs):
    """Mirror of inStrain.profile.profile_bam (profile/__init__.py:7-18).

    bam: path of a sorted BAM.  kwargs: the CLI's flags (min_cov, min_freq, min_snp, rarefied_coverage, min_read_ani,
    min_mapq, max_insert_relative, min_insert, pairing_filter, skip_mm_profiling, window_length, store_everything)
    plus `s2s` (scaffold -> upper-cased sequence, controller.py:337), `null_model` (dict, snv_utilities.py:14-38),
    optionally `ctx` (an engine.Context to reuse), `device`, `scaffold_tables` (dict that receives every scaffold's
    cumulative_scaffold_table from the device summaries), `logs` (list that receives the failure lines),
    `gene_file` (prodigal .fna) or `genes` ((scaff2geneinfo, scaff2gene2sequence)) with `gene_tables` (dict that receives genes_table,
    genes_coverage, genes_clonality, genes_SNP_count and SNP_mutation_types: the gene pass, gene_profile.py, on every batch),
    `stb` (scaffold -> genome, a dict or the path of a two-column tab-separated file) with `genome_tables` (dict that receives
    genome_info, scaffold2bin and bin2length: genomeUtilities.genomeLevel_from_IS from per-batch device roll-ups,
    genome_utilities.GenomeTables; scaffolds the stb does not name are left out, a genome may span batches; without `stb` no such call is made;
    its iRep / iRep_GC_corrected columns come from an engine.IRep that gets every batch and is finished once; `irep=False` skips all of
    that, `irep_accessory=True` also puts `iRep_accessory` into genome_tables: one row per genome of kept_windows, avg_cov, r2, fragMbp,
    unfiltered_raw_iRep, iRep_GC_corrected and unfiltered_iRep),
    `compare_set` (a compare.SampleSet on the same ctx) with `compare_sample` (this BAM's name in it, default: the path): every batch's
    sketch is added to the set before its slot is released (SampleSet.add_batch; without `compare_set` no such call is made),
    `pool_set` (a compare.SampleSet(pooling=True) whose pool_sites() has run) with `pool_sample` (default: the path): the second pass of
    SNV pooling -- every batch's slot is handed to SampleSet.pool_add before its release; a run with one mm bin then opens its pipe
    with want_counts (without `pool_set` nothing changes),
    `read_tables` (dict that receives `mapping_info`, the reference's read report over all wanted scaffolds -- filter_reads.mapping_info,
    made right after the read filter and before anything is dropped -- and `scaffolds_removed`, name -> reason; with `stb` and
    `genome_tables` genome_info then carries the reads_* columns and filtered_read_pair_count), `min_scaffold_reads` /
    `min_genome_coverage` (needs `stb`) / `database_mode` (= min_read_ani 0.92, skip_mm_profiling, min_genome_coverage 1,
    controller.py:210-214): the scaffold filters that read the report (filter_reads.filter_scaffolds); a scaffold they drop leaves the plan
    and the handle (BamFile.drop_refs) before the mm levels and the batches are made -- no SplitObject, no failure line; when nothing is
    left the result is {} and one error line.  With `sR2M` no filter runs here: read_tables stays empty and the three keywords raise
    ValueError (all of them off by default: a call without them does what it did),
    `batch_positions` / `batch_reads` (size of a device batch; `batch_observations` is accepted as 150 x batch_reads), `pipe_depth` (device batches in flight: the front end
    prepares batch k + 1 while batch k is profiled and its tables are cut), `stats` (dict that receives stage times).
    The BAM's reads go to the device as read segments (isx_pipe_submit_bam on a read-level pipe): the host never expands a
    read into per-base records.
    Returns {"scaffold.split": SplitObject} = Sprofile_dict (profile_utilities.py:85)."""
    s2s, null_model, logs = kwargs['s2s'], kwargs['null_model'], kwargs.get('logs')
    opt = profile_options(kwargs)
    out = {}
    stage = _StageClock(kwargs.get('stats'))
    own_ctx = kwargs.get('ctx') is None
    own_bf = kwargs.get('bamfile') is None           # a caller's handle may already hold the scan (dist.profile_bam_sharded)
    ctx = bf = run = helpers = gset = irep = None
    codes_of, layouts = [], []
    if kwargs.get('genes') is None and kwargs.get('gene_file'):        # a gene file the run cannot use is the caller's error, not a split's
        kwargs['genes'] = gene_profile.parse_genes(kwargs['gene_file'])
    scaffold_filters = bool(opt.min_scaffold_reads or opt.min_genome_coverage)
    if sR2M is not None and (scaffold_filters or kwargs.get('database_mode')):
        raise ValueError("min_scaffold_reads / min_genome_coverage / database_mode read the report of the built-in read filter: "
                         "with sR2M the controller has already filtered")
    if opt.min_genome_coverage and kwargs.get('stb') is None:          # the reference asserts here (controller.py:216-218)
        raise ValueError("If you adjust the minimum genome coverage, you need to provide an .stb!")
    rdb = None
    try:
        ctx = kwargs.get('ctx') or engine.Context(opt.device)
        ctx.set_null_model(*null_model_lut(null_model))
        gset = gene_profile.start_genes(ctx, kwargs)
        bf = kwargs.get('bamfile') or engine.BamFile(bam, threads=opt.host_threads)
        refs = bf.refs()
        plan, failed = select_scaffolds(refs, s2s, fasta_db, opt.window_length, bam)
        for name, (e, n_lines) in failed.items():
            _fail(logs, name, range(n_lines), e)
        stage("plan_ms")
        if not plan:
            return out
        # the scaffolds' sequence codes are made by helper threads while the front end scans the file (its passes run without
        # the GIL); the same helpers later set the pipe up and lay the groups out
        from concurrent.futures import ThreadPoolExecutor
        helpers = ThreadPoolExecutor(2)
        codes_of.extend(helpers.submit(_encode_scaffold, s2s[name]) for _, name, _ in plan)
        switch_threads = own_bf and opt.host_threads > 0 and opt.scan_threads != opt.host_threads
        if switch_threads:
            bf.set_threads(opt.scan_threads)
        bf.scan(part=opt.scan_part)
        stage("scan_ms")
        wanted_tids = choose_read_pairs(bf, plan, len(refs), sR2M, opt)
        if sR2M is None and (opt.read_tables is not None or scaffold_filters):
            stb = genome_utilities.parse_stb(kwargs['stb']) if kwargs.get('stb') is not None else None
            rdb, removed, keep = read_report_step(bf, plan, refs, wanted_tids, opt, stb)
            if opt.read_tables is not None:
                opt.read_tables['mapping_info'], opt.read_tables['scaffolds_removed'] = rdb, removed
            if len(keep) < len(plan):               # the reference never schedules them: no SplitObject, no failure line
                plan = [plan[k] for k in keep]
                codes_of[:] = [codes_of[k] for k in keep]
            if not plan:
                line = "No scaffolds passed initial filtering based on numbers of mapped reads"      # controller.py:319-321
                logging.error(line)
                if logs is not None:
                    logs.append(line)
                return out
        n_mm, mm_values, mm_clamped = mm_levels(bf, opt.skip_mm, opt.strict)
        reads_per_ref, _ = bf.ref_counts()
        if not opt.store_everything:                # (--store_everything keys read_to_snvs by read name: the names stay)
            bf.drop_names()
        if switch_threads:
            bf.set_threads(opt.host_threads)
        stage("filter_ms")
        # batches of whole scaffolds under a position / read budget; the reference groups its commands by estimated cost the same
        # way (profile_controller.py:436-457)
        est_segs = estimate_segments(bf.info, reads_per_ref, plan)
        item_groups = idist.pack_batches([refs[tid][1] for tid, _, _ in plan], est_segs, opt.batch_positions, opt.batch_segs)
        depth = pipe_depth_of(opt, len(item_groups))
        genomes = None
        if kwargs.get('stb') is not None:
            genomes = genome_utilities.GenomeTables(kwargs['stb'], {name: len(seq) for name, seq in s2s.items()})      # scaffold2length
        irep_index = None
        if genomes is not None and kwargs.get('irep', True):
            i_names, i_lengths, i_genome = genomes.irep_scaffolds()
            if i_names:
                irep = engine.IRep(ctx, i_lengths, i_genome, len(genomes.genomes), mask_edges=genomes.mask_edges)
                irep_index = {name: i for i, name in enumerate(i_names)}
        make_pipe = functools.partial(open_pipe, ctx, opt, n_mm, depth)
        if kwargs.get('pool_set') is not None:
            make_pipe = functools.partial(open_pipe, ctx, opt, n_mm, depth, pool=True)
        run = _BatchRun(bf, plan, refs, opt, make_pipe, depth, codes_of, est_segs, out, stage,
                        bam=bam, mm_values=mm_values, mm_clamped=mm_clamped, gset=gset, logs=logs,
                        scaffold_tables=kwargs.get('scaffold_tables'), scaffold_levels=kwargs.get('scaffold_levels'), genomes=genomes,
                        compare_set=kwargs.get('compare_set'), compare_sample=kwargs.get('compare_sample', bam),
                        irep=irep, irep_index=irep_index, pool_set=kwargs.get('pool_set'), pool_sample=kwargs.get('pool_sample', bam))
        # the pipe (pinned staging, device arena: tens of ms) is set up by one helper thread while another lays the groups out
        # (sequence codes, split tables: Python + numpy) -- a group's layout is then ready when the group before it is being handed
        # over (isx_pipe_submit_bam runs without the GIL)
        pipe_f = helpers.submit(run.open_pipe, largest_need(item_groups, plan, refs, est_segs))
        layouts.extend(helpers.submit(run.layout, items) for items in item_groups)
        pipe_f.result()
        stage("setup_ms")
        run.run(item_groups, layouts)
        if genomes is not None and kwargs.get('genome_tables') is not None:
            gt = kwargs['genome_tables']
            gt['scaffold2bin'], gt['bin2length'] = genomes.stb, genomes.bin2length
            if irep is not None:
                genomes.set_irep(irep.finish()[0])
                if kwargs.get('irep_accessory'):
                    gt['iRep_accessory'] = genomes.irep_accessory()
            if rdb is not None and opt.read_tables is not None:
                genomes.set_mapping_info(rdb)
            gt['genome_info'] = genomes.genome_info(skip_mm_profiling=opt.skip_mm)
        if gset is not None:
            gene_profile.finish_genes(gset, kwargs['gene_tables'] if kwargs.get('gene_tables') is not None else {})
        return out
    except Exception as e:
        # a failure of the call as a whole (unreadable BAM, a pair beyond the 128 mm levels a device batch holds, a device fault):
        # the reference's convention is per split (profile_utilities.py:104-111) -- with strict=True the caller gets the exception
        # itself instead of a partial dict and one log line, so "the call failed" cannot be mistaken for "no reads"
        if opt.strict:
            raise
        print(e)
        traceback.print_exc()
        t = time.strftime('%m-%d %H:%M')
        line = "\n{1} DEBUG FAILURE SplitException {0} batch\n".format(bam, t)
        logging.error(line)
        if logs is not None:
            logs.append(line)
        return out
    finally:
        if helpers is not None:
            helpers.shutdown(wait=True)
        if gset is not None:
            gset.close()
        if irep is not None:
            irep.close()
        # this call's own large arrays (sequence codes, group layouts) go before the helper thread below starts unmapping the pipe's
        # and the handle's gigabytes: both want the process' address-space lock
        del codes_of[:], layouts[:]
        dead = [o for o in (run.pipe if run is not None else None, bf if own_bf else None) if o is not None]
        if own_ctx and ctx is not None:
            for o in dead:
                o.close()
            ctx.close()
        elif dead:
            ctx.close_later(*dead)                   # a caller's context: unpinning / unmapping GBs is not on the caller's time
        stage("teardown_ms")
