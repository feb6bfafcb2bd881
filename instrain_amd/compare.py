"""Mirror of the per-pair body of `inStrain compare`:

    inStrain.readComparer.calc_mm2overlap(covT1, covT2, min_cov)                 readComparer.py:145-191
    inStrain.readComparer._calc_SNP_count_alternate(SNPtable1, SNPtable2, ...)   readComparer.py:205-290
    inStrain.readComparer._update_overlap_table(...)                             readComparer.py:437-502
    inStrain.readComparer.compare_scaffold (one sample pair)                     readComparer.py:35-143

Two samples profiled on the same scaffolds (two resident batches over the same flat space); the
position-sized work (cumulate covT over mm, threshold at min_cov, intersect / unite) and the SNP-table
comparison (highest-mm row per position, merge of the two samples' rows, consensus / population
verdicts, masking with the covered-in-both set per mm) run on the device (isx_compare_coverage /
isx_compare_scaffolds); the per-mm bookkeeping and the column naming here.

A whole sample set (every pair of every scaffold, compare_controller.py:611-658): SampleSet keeps a small per-sample sketch on the
device (isx_cmpset_*: one bit per position and level, the covT-key flags, the last SNV row of every position), so batches -- pipe
slots included -- can go as soon as they have been added; compare() then counts all pairs in one pass.  genome_wide() is
genomeUtilities._genome_wide_readComparer (genomeUtilities.py:739-800) after _add_stb (:430-448), on the host.

Strain clustering (strain_clusters.tsv; compare_utils.py:205-255 cluster_genome_strains): SampleSet.strain_clusters()
from the counters compare() left on the device, cluster_genome_strains() from a genome_wide / stored genomeWide_compare frame,
linkage_flat() from plain matrices -- all three through the same kernel (isx_cluster.hip); there is no host path that clusters.
"""
import ctypes as C
import itertools
import time

import numpy as np

from . import _lib
from ._lib import check


def calc_mm2overlap(batch1, batch2, scaffold_bounds, min_cov=5):
    """-> (list over scaffolds of {mm: n_covered_in_both}, list of {mm: coverage}, device ms).
    Levels = union of the two samples' covT keys on that scaffold, like the reference; coverage =
    len(coveredInBoth) / len(coveredInEither) (0 when nothing is covered)."""
    sb = np.ascontiguousarray(scaffold_bounds, dtype=np.int64)
    M = max(batch1.n_mm_bins, batch2.n_mm_bins)
    out = np.zeros((len(sb) - 1, M), dtype=_lib.COMPARE_LEVEL_DT)
    ms = C.c_float(0)
    check(batch1.lib.isx_compare_coverage(batch1.h, batch2.h, len(sb) - 1, sb.ctypes.data, int(min_cov), out.ctypes.data, C.byref(ms)))
    mm2overlap, mm2coverage = [], []
    for rows in out:
        o, c = {}, {}
        for r in rows:
            if r["present_a"] or r["present_b"]:
                o[int(r["mm"])] = int(r["both"])
                c[int(r["mm"])] = r["both"] / r["either"] if r["either"] > 0 else 0
        mm2overlap.append(o)
        mm2coverage.append(c)
    return mm2overlap, mm2coverage, ms.value


def _comparison_row(r, length, scaffold, name1, name2):
    """one COMPARE_LEVEL_DT record as the reference's comparisonsTable row (readComparer.py:437-502); the key order is the column order
    of every frame built from these rows"""
    bases = int(r["both"])
    snps, popsnps = int(r["consensus_snps"]), int(r["population_snps"])
    return {"mm": int(r["mm"]), "scaffold": scaffold, "name1": name1, "name2": name2,
            "coverage_overlap": r["both"] / r["either"] if r["either"] > 0 else 0,
            "compared_bases_count": bases, "percent_genome_compared": bases / length, "length": length,
            "consensus_SNPs": snps, "population_SNPs": popsnps,
            "conANI": (bases - snps) / bases if bases else np.nan,
            "popANI": (bases - popsnps) / bases if bases else np.nan}


def _mdb(raw, offsets, failed):
    """COMPARE_SNP_DT rows as the Mdb dict: offsets = first gpos of every scaffold (ascending); rows on `failed` scaffolds are left out"""
    scaf = np.searchsorted(offsets, raw["gpos"].astype(np.int64), side="right") - 1
    if failed:
        ok = ~np.isin(scaf, sorted(failed))
        raw, scaf = raw[ok], scaf[ok]
    return {"raw": raw, "scaffold": scaf, "position": raw["gpos"].astype(np.int64) - offsets[scaf]}


def _batch_args(who, index, batch_scaffold_names, batch_bounds):
    """-> (bounds int64, ids int32: scaffold of the set or -1) of a batch handed to a SampleSet; `who` heads the ValueError"""
    bb = np.ascontiguousarray(batch_bounds, dtype=np.int64)
    ids = np.array([index.get(n, -1) for n in batch_scaffold_names], dtype=np.int32)
    if len(bb) != len(ids) + 1:
        raise ValueError("%s: batch_bounds has one entry more than the batch has scaffolds" % who)
    return bb, ids


BASES = np.array(["A", "C", "T", "G", "N"])
POOL_CLASSES = ("DivergentSite", "SNS", "SNV", "con_SNV", "pop_SNV")        # the <class>_count columns of PMdb (polymorpher.py:492)


def compare_scaffolds(batch1, batch2, scaffold_bounds, scaffold_names=None, name1="sample1", name2="sample2",
                      min_cov=5, min_freq=0.05, store_mismatch_locations=False):
    """One sample pair of compare_scaffold (readComparer.py:80-121) for every scaffold of the flat space.
    -> (Cdb rows: list of dicts with the reference's columns, ascending (scaffold, mm);
        Mdb: structured array of mismatch locations (COMPARE_SNP_DT + 'scaffold' index, 'position') or None;
        device ms).
    A scaffold on which the reference itself fails (KeyError on an N reference base, see
    include/instrain_amd.h) is reported as {'scaffold': ..., 'failed': True} like its results=None."""
    sb = np.ascontiguousarray(scaffold_bounds, dtype=np.int64)
    n_scaf = len(sb) - 1
    names = list(scaffold_names) if scaffold_names is not None else list(range(n_scaf))
    M = max(batch1.n_mm_bins, batch2.n_mm_bins)
    out = np.zeros((n_scaf, M), dtype=_lib.COMPARE_LEVEL_DT)
    ms, n_rows = C.c_float(0), C.c_int64(0)
    check(batch1.lib.isx_compare_scaffolds(batch1.h, batch2.h, n_scaf, sb.ctypes.data, int(min_cov), float(min_freq),
                                           out.ctypes.data, C.byref(n_rows), C.byref(ms)))
    table, failed = [], set()
    for i, rows in enumerate(out):
        mLen = int(sb[i + 1] - sb[i])
        if (rows["consensus_snps"] == -2).any():
            table.append({"scaffold": names[i], "failed": True})
            failed.add(i)
            continue
        for r in rows:
            if not (r["present_a"] or r["present_b"]):
                continue
            table.append(_comparison_row(r, mLen, names[i], name1, name2))
    mdb = None
    if store_mismatch_locations:
        raw = np.zeros(n_rows.value, dtype=_lib.COMPARE_SNP_DT)
        if n_rows.value:
            check(batch1.lib.isx_compare_fetch_snps(batch1.h, raw.ctypes.data))
        mdb = _mdb(raw, sb, failed)
    return table, mdb, ms.value


# ---- a whole sample set (isx_cmpset_*) ----
def set_layout(scaffold_lengths):
    """first 64-position word of every scaffold in a set's own position space, then the total (isx_cmpset_layout; host only)"""
    ln = np.ascontiguousarray(scaffold_lengths, dtype=np.int64)
    off = np.zeros(len(ln) + 1, dtype=np.int64)
    check(_lib.load().isx_cmpset_layout(len(ln), ln.ctypes.data, off.ctypes.data))
    return off


def tile_directory(scaffold_lengths, tile_words):
    """the pair kernel's tiles (word0, n_words, scaffold): runs of at most tile_words words that never cross a scaffold (host only)"""
    lib = _lib.load()
    ln = np.ascontiguousarray(scaffold_lengths, dtype=np.int64)
    n = lib.isx_cmpset_tiles(len(ln), ln.ctypes.data, int(tile_words), None)
    if n < 0:
        check(int(n))
    tiles = np.zeros(n, dtype=_lib.CMPSET_TILE_DT)
    lib.isx_cmpset_tiles(len(ln), ln.ctypes.data, int(tile_words), tiles.ctypes.data)
    return tiles


def level_map(sample_mm_values, cap_axis=_lib.CMPSET_MAX_LEVELS):
    """-> (axis: sorted union of the samples' real mm values, map[sample, axis level] = the sample's own highest level with a value
    <= the axis level's, -1 = none yet) (isx_cmpset_level_map; host only)"""
    n_levels = np.array([len(v) for v in sample_mm_values], dtype=np.int32)
    flat = np.ascontiguousarray(np.concatenate([np.asarray(v, dtype=np.int32) for v in sample_mm_values] + [np.zeros(0, np.int32)]))
    axis, n_axis = np.zeros(cap_axis, dtype=np.int32), C.c_int32(0)
    lmap = np.zeros((len(n_levels), cap_axis), dtype=np.int32)
    check(_lib.load().isx_cmpset_level_map(len(n_levels), n_levels.ctypes.data, flat.ctypes.data, int(cap_axis), axis.ctypes.data,
                                           C.byref(n_axis), lmap.ctypes.data))
    return axis[:n_axis.value].copy(), lmap[:, :n_axis.value].copy()


# ---- stored profiles (compare_controller.py:520-577: covT of raw_data/covT.hd5 and the cumulative_snv_table) ----
SNV_OLD_NAMES = {"conBase": "con_base", "refBase": "ref_base", "varBase": "var_base", "baseCoverage": "position_coverage"}  # (:544-546)
_BASE_CODE = {"A": 0, "C": 1, "T": 2, "G": 3, "N": 4}


def _whole(a, what, top):
    """an array of whole numbers within 0..top -> int64; ValueError otherwise (NaN, fractions, negatives, text)"""
    a = np.asarray(a)
    if a.dtype.kind == "f":
        if not np.isfinite(a).all() or (a != np.floor(a)).any():
            raise ValueError("pack_profile: %s holds NaN or a value that is no whole number" % what)
    elif a.dtype.kind not in "iu":
        raise ValueError("pack_profile: %s is not numeric (%s)" % (what, a.dtype))
    if a.size and (a.min() < 0 or a.max() > top):
        raise ValueError("pack_profile: %s outside 0..%d" % (what, top))
    return a.astype(np.int64)


def _series(ser, what, length):
    """one covT series (a pd.Series of values indexed by position, or a (positions, values) tuple) -> ascending uint32 pairs"""
    pos, val = ser if isinstance(ser, tuple) else (ser.index.to_numpy(), ser.to_numpy())
    pos, val = _whole(pos, what + " positions", length - 1), _whole(val, what + " values", 0xFFFFFFFF)
    if pos.shape != val.shape or pos.ndim != 1:
        raise ValueError("pack_profile: %s has not one value per position" % what)
    if len(pos) > 1 and (pos[1:] <= pos[:-1]).any():
        order = np.argsort(pos, kind="stable")
        pos, val = pos[order], val[order]
        if (pos[1:] == pos[:-1]).any():
            raise ValueError("pack_profile: %s names a position twice" % what)
    return pos.astype(np.uint32), val.astype(np.uint32)


def _snv_flags(db):
    """the snv_flags of isx_cmpset_add_profile_pool for the rows of a cumulative_snv_table: class code | cryptic << 3"""
    from .profile.snv_utilities import CLASSES
    for col in ("class", "cryptic"):
        if col not in db.columns:
            raise ValueError("pack_profile: pooling needs the SNV table's column %s" % col)
    code = np.array([CLASSES.index(c) if c in CLASSES else -1 for c in db["class"].astype(object)], dtype=np.int64)
    if (code < 0).any():
        raise ValueError("pack_profile: the SNV table's column class holds %r"
                         % sorted({str(c) for c, k in zip(db["class"].astype(object), code) if k < 0}))
    cryptic = db["cryptic"].to_numpy()
    if cryptic.dtype.kind not in "biuf" or not np.isin(cryptic, (0, 1)).all():
        raise ValueError("pack_profile: the SNV table's column cryptic holds other values than True / False")
    return (code | (cryptic.astype(np.int64) << 3)).astype(np.uint8)


def pool_window(site_positions, owned):
    """the columns [lo, hi) the reference piles up to pull one (sample, scaffold) (polymorpher.py:293: max(min(p) - 1, 0) to max(p) + 1
    over the sites p the sample does not own) -> (lo, hi, n), None when there is nothing to pull.  site_positions: the scaffold's
    sites as positions on the scaffold; owned: bool per site"""
    p = np.asarray(site_positions, dtype=np.int64)[~np.asarray(owned, dtype=bool)]
    if len(p) == 0:
        return None
    return max(int(p.min()) - 1, 0), int(p.max()) + 1, int(len(p))


def pack_profile(index, lengths, covT, snv_table, mm_values=None, pool=False):
    """A stored profile as the arrays of isx_cmpset_add_profile; numpy only, no device.  pool: also "flags" (uint8 per kept SNV row: the
    snv_flags of isx_cmpset_add_profile_pool, from the table's `class` and `cryptic` columns -- a table without them, or with a class
    name outside profile.snv_utilities.CLASSES, raises ValueError naming the column).
    index: scaffold name -> scaffold of the set; lengths: the set's lengths.  covT: {scaffold: {mm: pd.Series(values, index=positions)}}
    (emitters.load_special; (positions, values) tuples are taken too).  snv_table: the cumulative_snv_table (columns scaffold, position,
    mm, con_base, ref_base, var_base, allele_count, A, C, T, G; the old names conBase / refBase / varBase / baseCoverage are renamed as
    the reference does), an empty frame or None.  mm_values: the sample's levels, None = the sorted union of the covT keys over the
    scaffolds the set names.
    -> {"scaffolds": names, in set order; "ids" int32; "levels" int32; "present" uint8 [scaffold, level]; "offsets" int64 (CSR over
    (scaffold, level)); "positions", "values" uint32; "snv" PROFILE_SNV_DT}.  Scaffolds the set does not name or whose covT has no key
    are left out, SNV rows on them and on scaffolds without a covT entry are dropped (the reference never pairs such a sample there).
    A series whose index does not ascend is sorted; a position twice or beyond the set's length, a negative / fractional / NaN value, an
    unknown base letter or a position_coverage other than A + C + T + G raise ValueError."""
    lengths = np.asarray(lengths, dtype=np.int64)
    kept = sorted((index[n], n) for n, d in (covT or {}).items() if n in index and len(d))
    names = [n for _, n in kept]
    keys = {n: {int(mm): ser for mm, ser in covT[n].items()} for n in names}
    union = sorted({mm for d in keys.values() for mm in d})
    if mm_values is None:
        levels = np.array(union, dtype=np.int32)
    else:
        levels = np.array(mm_values, dtype=np.int32).reshape(-1)
        if len(levels) > 1 and (levels[1:] <= levels[:-1]).any():
            raise ValueError("pack_profile: mm_values must ascend strictly")
        missing = sorted(set(union) - set(levels.tolist()))
        if missing:
            raise ValueError("pack_profile: covT has the keys %s, which mm_values does not name" % missing)
    L = len(levels)
    present = np.zeros((len(names), L), dtype=np.uint8)
    offsets = np.zeros(len(names) * L + 1, dtype=np.int64)
    pos_parts, val_parts = [np.zeros(0, np.uint32)], [np.zeros(0, np.uint32)]
    for i, n in enumerate(names):
        for k, mm in enumerate(levels.tolist()):
            n_here = 0
            if mm in keys[n]:
                present[i, k] = 1
                p, v = _series(keys[n][mm], "covT[%r][%d]" % (n, mm), int(lengths[index[n]]))
                pos_parts.append(p)
                val_parts.append(v)
                n_here = len(p)
            offsets[i * L + k + 1] = offsets[i * L + k] + n_here
    out = {"scaffolds": names, "ids": np.array([i for i, _ in kept], dtype=np.int32), "levels": levels, "present": present,
           "offsets": offsets, "positions": np.concatenate(pos_parts), "values": np.concatenate(val_parts),
           "snv": np.zeros(0, dtype=_lib.PROFILE_SNV_DT)}
    if pool:
        out["flags"] = np.zeros(0, dtype=np.uint8)
    if snv_table is None or len(snv_table) == 0:
        return out
    db = snv_table.rename(columns=SNV_OLD_NAMES)
    need = ["scaffold", "position", "mm", "con_base", "ref_base", "var_base", "allele_count", "A", "C", "T", "G"]
    lacking = [c for c in need if c not in db.columns]
    if lacking:
        raise ValueError("pack_profile: the SNV table has no column %s" % ", ".join(lacking))
    local = {n: i for i, n in enumerate(names)}
    sc = np.array([local.get(n, -1) for n in db["scaffold"].astype(object)], dtype=np.int64)
    db = db[sc >= 0]
    sc = sc[sc >= 0]
    rows = np.zeros(len(db), dtype=_lib.PROFILE_SNV_DT)
    rows["scaffold"] = sc
    position = _whole(db["position"].to_numpy(), "SNV positions", 0xFFFFFFFF)
    if (position >= lengths[out["ids"][sc]]).any():
        raise ValueError("pack_profile: an SNV row lies beyond its scaffold")
    rows["position"] = position
    rows["mm"] = _whole(db["mm"].to_numpy(), "SNV mm", 65535)
    rows["allele_count"] = _whole(db["allele_count"].to_numpy(), "allele_count", 255)
    for col, top in (("con_base", 3), ("ref_base", 4), ("var_base", 3)):
        code = np.array([_BASE_CODE.get(b, 9) for b in db[col].astype(object)], dtype=np.int64)
        if (code > top).any():
            raise ValueError("pack_profile: %s holds %r" % (col, sorted({str(b) for b, c in zip(db[col].astype(object), code) if c > top})))
        rows[col] = code
    for j, b in enumerate("ACTG"):
        rows["cnt"][:, j] = _whole(db[b].to_numpy(), "the SNV table's column " + b, 0xFFFFFFFF)
    if "position_coverage" in db.columns:
        pc = db["position_coverage"].to_numpy()
        if pc.dtype.kind not in "iuf" or (pc != rows["cnt"].astype(np.int64).sum(axis=1)).any():
            raise ValueError("pack_profile: position_coverage is not A + C + T + G in every row")
    out["snv"] = rows
    if pool:
        out["flags"] = _snv_flags(db)
    return out


def _scaffold_profiles(profiles):
    """scaffold profiles as they come, or profile_bam's {"scaffold.split": SplitObject} merged per scaffold (from_splits)"""
    from .profile import profile_utilities as pu
    items = list(profiles.values()) if isinstance(profiles, dict) else list(profiles)
    if all(hasattr(P, "cumulative_scaffold_table") for P in items):
        return items
    by = {}
    for S in items:
        by.setdefault(S.scaffold, []).append(S)
    return [pu.scaffold_profile.from_splits(sorted(parts, key=lambda S: S.split_number)) for parts in by.values()]


def store_sample(folder, profiles):
    """covT.hd5 and cumulative_snv_table.csv.gz of a sample under `folder` (the raw_data folder of the reference's profile, under its
    names, through profile.emitters).  profiles: the sample's scaffold profiles (scaffold_profile.from_splits), or what profile_bam
    returns.  -> the two paths"""
    import os
    import pandas as pd
    from .profile import emitters
    profs = _scaffold_profiles(profiles)
    covT = {P.scaffold: P.covT for P in profs if P.covT}
    tables = [P.cumulative_snv_table for P in profs if getattr(P, "cumulative_snv_table", None) is not None and len(P.cumulative_snv_table)]
    sdb = pd.concat(tables).reset_index(drop=True) if tables else pd.DataFrame()
    os.makedirs(folder, exist_ok=True)
    return (emitters.store_special(covT, os.path.join(folder, "covT")),
            emitters.store_pandas(sdb, os.path.join(folder, "cumulative_snv_table")))


def load_sample(folder, scaffolds=None):
    """-> (covT, snv_table) of a stored sample: `folder` holds covT.hd5 and cumulative_snv_table.csv.gz -- written by store_sample, or the
    raw_data folder of a profile the reference wrote.  scaffolds: load only these."""
    import os
    import pandas as pd
    from .profile import emitters
    covT = emitters.load_special(os.path.join(folder, "covT.hd5"), scaffolds=None if scaffolds is None else set(scaffolds))
    try:
        sdb = emitters.load_pandas(os.path.join(folder, "cumulative_snv_table.csv.gz"))
    except pd.errors.EmptyDataError:
        sdb = pd.DataFrame()
    if scaffolds is not None and "scaffold" in sdb.columns:
        sdb = sdb[sdb["scaffold"].isin(set(scaffolds))].reset_index(drop=True)
    return covT, sdb


class SampleSet:
    """The samples of one `inStrain compare` run on the device.  scaffold_names / scaffold_lengths: the scaffolds to compare, in the
    order of the output.  Samples are numbered in the order of their first add_batch / add_profile."""

    def __init__(self, ctx, scaffold_names, scaffold_lengths, min_cov=5, pooling=False):
        """pooling: also keep every sample's own SNV rows for pool_sites() / pool_add() / pooled_tables() (`compare --bams`)"""
        self.ctx, self.lib = ctx, ctx.lib
        self.pooling = bool(pooling)
        self.n_pool_sites = None                                # sites of the last pool_sites(); None: none since the last add_batch
        self.pool_device_ms, self.pool_raw = 0.0, None
        self.names = list(scaffold_names)
        self.lengths = np.ascontiguousarray(scaffold_lengths, dtype=np.int64)
        if len(self.names) != len(self.lengths) or len(set(self.names)) != len(self.names):
            raise ValueError("SampleSet: one length per scaffold, every scaffold once")
        self.index = {n: i for i, n in enumerate(self.names)}
        self.offsets = set_layout(self.lengths) * 64            # first set position of every scaffold
        self.samples = []
        self._have = {}                                         # sample -> scaffolds of the set it has brought
        self.profile_device_ms = 0.0                            # of the last add_profile()
        self.failed = set()                                     # scaffolds on which a pair of the last compare() failed
        self.device_ms, self.levels = 0.0, None
        self.cluster_genomes, self.cluster_status, self.cluster_labels, self.cluster_device_ms = [], None, None, 0.0   # of the last strain_clusters()
        h = C.c_void_p()
        check(self.lib.isx_cmpset_create(ctx.h, len(self.names), self.lengths.ctypes.data, int(min_cov), C.byref(h)))
        self.h = h
        ctx._adopt(self)
        if self.pooling:
            check(self.lib.isx_cmpset_pool_enable(self.h))

    def add_batch(self, sample_name, batch, batch_scaffold_names, batch_bounds, mm_values=None):
        """what `batch` (a run Batch or a collected pipe slot) holds of the sample; scaffolds the set does not name are skipped.
        mm_values: the real mm of every device level (profile_bam's mm_values), None = level k is mm k.  The batch may be closed /
        its slot released as soon as this returns."""
        bb, ids = _batch_args("add_batch", self.index, batch_scaffold_names, batch_bounds)
        mmv = None if mm_values is None else np.ascontiguousarray(mm_values, dtype=np.int32)
        if mmv is not None and len(mmv) != batch.n_mm_bins:
            raise ValueError("add_batch: one mm value per level of the batch")
        known = sample_name in self.samples
        check(self.lib.isx_cmpset_add(self.h, self.samples.index(sample_name) if known else len(self.samples), batch.h, len(ids),
                                      bb.ctypes.data, ids.ctypes.data, None if mmv is None else mmv.ctypes.data))
        if not known:                                           # (a refused batch leaves the set as it was)
            self.samples.append(sample_name)
        self.n_pool_sites = None                                # (the library has dropped its pooling state)
        self._have.setdefault(sample_name, set()).update(ids[ids >= 0].tolist())

    def add_profile(self, sample_name, covT, snv_table=None, mm_values=None, max_entries=1 << 26):
        """a sample from its STORED profile (load_sample, or the reference's covT and cumulative_snv_table) instead of a resident batch:
        the same sketch, so compare() and everything behind it cannot tell how a sample arrived, and one sample may come scaffold by
        scaffold through both.  covT, snv_table, mm_values: see pack_profile.  The packed profile goes to the device in chunks of whole
        scaffolds of at most max_entries coverage entries (a larger scaffold goes alone), which bounds the host staging and the device
        scratch.  Refused as a whole (the set stays as it was): a set with pooling, other levels than the sample's earlier calls, a
        scaffold the sample already has.  self.profile_device_ms: the event-timed device passes of the call."""
        self.add_packed(sample_name, pack_profile(self.index, self.lengths, covT, snv_table, mm_values), max_entries)

    def add_packed(self, sample_name, p, max_entries=1 << 26):
        """add_profile's second half: p = pack_profile(self.index, self.lengths, ...) of the sample, made earlier"""
        if self.pooling:                                        # (the library's own refusal, also for a profile with no scaffold of the set)
            raise _lib.IsxError(-6, "add_profile: the own rows of a set with pooling need the class / cryptic columns of the SNV table: "
                                    "add_profile_pooled takes them")
        self._add_packed(sample_name, p, max_entries, False)

    def add_profile_pooled(self, sample_name, covT, snv_table, mm_values=None, max_entries=1 << 26):
        """add_profile for a set with pooling (`inStrain compare -i ... --bams`): the stored cumulative_snv_table -- with its `class` and
        `cryptic` columns -- also gives the sample's own rows of pool_sites(), exactly as add_batch leaves them (PoolController.__init__,
        polymorpher.py:53-70).  The pull then needs the sample's reads: pool_stored() / pool_add_obs() from its BAM, or pool_add() /
        profile_bam(pool_set=...).  A set without pooling refuses (-6)."""
        if not self.pooling:
            raise _lib.IsxError(-6, "add_profile_pooled: the set keeps no pool rows (SampleSet(pooling=True)); add_profile is its call")
        self._add_packed(sample_name, pack_profile(self.index, self.lengths, covT, snv_table, mm_values, pool=True), max_entries, True)

    def _add_packed(self, sample_name, p, max_entries, pool):
        known = sample_name in self.samples
        sample = self.samples.index(sample_name) if known else len(self.samples)
        self.profile_device_ms = 0.0
        again = sorted(set(p["ids"].tolist()) & self._have.get(sample_name, set()))
        if again:                                               # (the library would refuse only the chunk that holds it)
            raise _lib.IsxError(-6, "add_profile: scaffold %s of sample %r was added before" % (self.names[again[0]], sample_name))
        L, off = len(p["levels"]), p["offsets"]
        per_scaffold = off[L::L] - off[:-1:L] if L else np.zeros(0, np.int64)
        i0, n = 0, len(p["ids"])
        while i0 < n:
            i1, held = i0 + 1, int(per_scaffold[i0])
            while i1 < n and held + int(per_scaffold[i1]) <= max_entries:
                held += int(per_scaffold[i1])
                i1 += 1
            e0, e1 = int(off[i0 * L]), int(off[i1 * L])
            sub_off = np.ascontiguousarray(off[i0 * L:i1 * L + 1] - e0)
            positions, values = np.ascontiguousarray(p["positions"][e0:e1]), np.ascontiguousarray(p["values"][e0:e1])
            ids, present = np.ascontiguousarray(p["ids"][i0:i1]), np.ascontiguousarray(p["present"][i0:i1])
            here = (p["snv"]["scaffold"] >= i0) & (p["snv"]["scaffold"] < i1)
            snv = p["snv"][here].copy()
            snv["scaffold"] -= i0
            ms = C.c_float(0)
            args = (self.h, sample, i1 - i0, ids.ctypes.data, L, p["levels"].ctypes.data, present.ctypes.data, sub_off.ctypes.data,
                    positions.ctypes.data, values.ctypes.data, len(snv), snv.ctypes.data)
            if pool:                                            # the flags follow their rows into the chunk
                flags = np.ascontiguousarray(p["flags"][here])
                check(self.lib.isx_cmpset_add_profile_pool(*args, flags.ctypes.data, C.byref(ms)))
            else:
                check(self.lib.isx_cmpset_add_profile(*args, C.byref(ms)))
            self.profile_device_ms += ms.value
            i0 = i1
        if not known:
            self.samples.append(sample_name)
        self.n_pool_sites = None
        self._have.setdefault(sample_name, set()).update(p["ids"].tolist())

    def compare(self, min_freq=0.05, logs=None):
        """-> the comparisonsTable rows (the columns of compare_scaffolds) of every pair of samples over every scaffold both have,
        ordered by (scaffold, pair as itertools.combinations, mm).  A scaffold on which ANY pair fails gives no row at all and one
        failure line in `logs` (compare_utils.py:86-107: results = None for the whole scaffold)."""
        n_s, n_a = C.c_int32(0), C.c_int32(0)
        check(self.lib.isx_cmpset_axis(self.h, C.byref(n_s), C.byref(n_a), None))
        pairs = list(itertools.combinations(range(n_s.value), 2))
        out = np.zeros((len(pairs), len(self.names), n_a.value), dtype=_lib.COMPARE_LEVEL_DT)
        ms = C.c_float(0)
        check(self.lib.isx_cmpset_compare(self.h, float(min_freq), out.size, out.ctypes.data, C.byref(ms)))
        self.device_ms = ms.value
        self.levels = out                                       # the device's rows as they came: [pair, scaffold, axis level]
        by_scaffold = out.transpose(1, 0, 2)
        present = (by_scaffold["present_a"] != 0) | (by_scaffold["present_b"] != 0)
        failed = (by_scaffold["consensus_snps"] == -2).any(axis=(1, 2)) if out.size else np.zeros(len(self.names), bool)
        self.failed = set(np.flatnonzero(failed).tolist())
        for sc in sorted(self.failed):
            have = sorted({i for p in np.flatnonzero(present[sc].any(axis=1)) for i in pairs[p]})
            line = "\n{1} DEBUG FAILURE CompareScaffold {0} {2}\n".format(self.names[sc], time.strftime('%m-%d %H:%M'),
                                                                         str([self.samples[i] for i in have]))
            if logs is not None:
                logs.append(line)
        present[failed] = False
        table = []
        for sc, p, a in np.argwhere(present):
            table.append(_comparison_row(by_scaffold[sc, p, a], int(self.lengths[sc]), self.names[sc], self.samples[pairs[p][0]],
                                         self.samples[pairs[p][1]]))
        return table

    def mismatch_locations(self, name1, name2):
        """the mismatch rows (--store_mismatch_locations) of one pair, as compare_scaffolds' Mdb: {'raw': COMPARE_SNP_DT rows sorted
        by (mm, set position), 'scaffold': index in the set, 'position': on the scaffold}; name1 is the sample added first.  Needs a
        compare() since the last add_batch; rows of its failed scaffolds are left out."""
        i, j = self.samples.index(name1), self.samples.index(name2)
        if i >= j:
            raise ValueError("mismatch_locations: name1 must be the sample that was added before name2")
        n = C.c_int64(0)
        check(self.lib.isx_cmpset_pair_snps(self.h, i, j, C.byref(n)))
        raw = np.zeros(n.value, dtype=_lib.COMPARE_SNP_DT)
        if n.value:
            check(self.lib.isx_cmpset_fetch_snps(self.h, raw.ctypes.data))
        return _mdb(raw, self.offsets, self.failed)

    # ---- SNV pooling (polymorpher.py PoolController; include/instrain_amd.h isx_cmpset_pool_*) ----
    def pool_sites(self):
        """after the last add_batch: the union of the samples' own SNV positions on every scaffold at least two samples have -> number
        of sites.  Every batch then goes through pool_add() once more (the reference goes back to the BAM)."""
        n = C.c_int64(0)
        check(self.lib.isx_cmpset_pool_sites(self.h, C.byref(n)))
        self.n_pool_sites = n.value
        return n.value

    def pool_site_positions(self):
        """the sites of the last pool_sites() as ascending set positions"""
        raw = np.zeros(self.n_pool_sites or 0, dtype=np.uint32)
        check(self.lib.isx_cmpset_pool_fetch_sites(self.h, raw.ctypes.data))
        return raw

    def pool_add(self, sample_name, batch, batch_scaffold_names, batch_bounds):
        """the all-level base counts of `batch` at the sites the sample does not own (get_pooling_counts); arguments as add_batch.  A
        one-level pipe slot needs the pipe's want_counts.  The batch may be closed / its slot released as soon as this returns."""
        bb, ids = _batch_args("pool_add", self.index, batch_scaffold_names, batch_bounds)
        if sample_name not in self.samples:
            raise ValueError("pool_add: sample %r was never added" % (sample_name,))
        check(self.lib.isx_cmpset_pool_add(self.h, self.samples.index(sample_name), batch.h, len(ids), bb.ctypes.data, ids.ctypes.data))

    # ---- the pull of a sample that came from a stored profile: observations of its BAM (isx_cmpset_pool_add_obs / _obs_done) ----
    def pool_plan(self, sample_name):
        """after pool_sites(): {scaffold name: (lo, hi, n_sites)} -- the columns [lo, hi) the reference would pile up for the sample
        (pool_window) and the sites in them it has to pull; scaffolds with nothing to pull are left out"""
        i = self.samples.index(sample_name)
        n = self.n_pool_sites or 0
        gpos = self.pool_site_positions().astype(np.int64)      # (no pool_sites() since the last add: the library refuses here)
        counts, meta = np.zeros((n, 4), dtype=np.uint32), np.zeros(n, dtype=np.uint8)
        check(self.lib.isx_cmpset_pool_fetch_sample(self.h, i, counts.ctypes.data, meta.ctypes.data))
        scaf = np.searchsorted(self.offsets, gpos, side="right") - 1
        plan = {}
        for sc in np.unique(scaf[(meta & _lib.POOL_META_HAS) != 0]).tolist():
            k = scaf == sc
            w = pool_window(gpos[k] - self.offsets[sc], (meta[k] & _lib.POOL_META_OWN) != 0)
            if w is not None:
                plan[self.names[sc]] = w
        return plan

    def pool_add_obs(self, sample_name, scaffold_names, obs, obs_offsets, gpos0=None):
        """pileup observations (engine.OBS_DT, host) of the sample's reads: region i = obs[obs_offsets[i]:obs_offsets[i + 1]] lies on
        scaffold_names[i], at position obs["gpos"] - gpos0[i] (None: 0, what BamFile.expand_region hands out).  Every level counts, at
        the sites the sample does not own; counts ADD, so a scaffold may come column window after column window -- but no column
        twice -- and is closed by pool_obs_done().  -> the event-timed device ms of the call"""
        if sample_name not in self.samples:
            raise ValueError("pool_add_obs: sample %r was never added" % (sample_name,))
        ids = np.array([self.index.get(n, -1) for n in scaffold_names], dtype=np.int32)
        off = np.ascontiguousarray(obs_offsets, dtype=np.int64)
        g0 = np.zeros(len(ids), dtype=np.int64) if gpos0 is None else np.ascontiguousarray(gpos0, dtype=np.int64)
        if len(off) != len(ids) + 1 or len(g0) != len(ids):
            raise ValueError("pool_add_obs: obs_offsets has one entry more than there are regions, gpos0 one per region")
        obs = np.ascontiguousarray(obs, dtype=_lib.OBS_DT)
        ms = C.c_float(0)
        check(self.lib.isx_cmpset_pool_add_obs(self.h, self.samples.index(sample_name), len(ids), ids.ctypes.data, g0.ctypes.data,
                                               off.ctypes.data, len(obs), obs.ctypes.data if len(obs) else None, C.byref(ms)))
        return ms.value

    def pool_obs_done(self, sample_name, scaffold_names=None):
        """the sample's scaffolds (None: every scaffold of its pool_plan()) have brought all their observations: pulled, a scaffold
        without any observation with zeros (polymorpher.py:306-308)"""
        if sample_name not in self.samples:
            raise ValueError("pool_obs_done: sample %r was never added" % (sample_name,))
        names = list(self.pool_plan(sample_name)) if scaffold_names is None else list(scaffold_names)
        ids = np.array([self.index.get(n, -1) for n in names], dtype=np.int32)
        check(self.lib.isx_cmpset_pool_obs_done(self.h, self.samples.index(sample_name), len(ids), ids.ctypes.data if len(ids) else None))

    def pooled_tables(self):
        """-> (DSTdb, PMdb) of polymorpher.py:397-448 / :471-551 as pandas frames.  DSTdb: index (sample, position), columns A C T G and
        the categorical `scaffold`, rows by (scaffold in set order, sample in insertion order, position).  PMdb: index position, the
        reference's columns.  A site no sample sees at >= 5 reads (the reference raises there) has sample_5x_detections 0."""
        import pandas as pd
        n_s, n_a = C.c_int32(0), C.c_int32(0)
        check(self.lib.isx_cmpset_axis(self.h, C.byref(n_s), C.byref(n_a), None))
        S = n_s.value
        n = self.n_pool_sites or 0                              # (None: the library refuses the call below)
        summary = np.zeros(n, dtype=_lib.POOL_SITE_DT)
        ms = C.c_float(0)
        try:
            check(self.lib.isx_cmpset_pool_summary(self.h, n, summary.ctypes.data, C.byref(ms)))
        except _lib.IsxError as e:                              # the library names the open (sample, scaffold) by index: add the names
            import re
            at = re.search(r"sample (\d+) has \d+ sites to pull on scaffold (\d+)", str(e))
            if e.code != -6 or at is None:
                raise
            raise _lib.IsxError(-6, "%s (sample %r, scaffold %s)" % (str(e).split(": ", 1)[-1], self.samples[int(at.group(1))],
                                                                     self.names[int(at.group(2))])) from None
        self.pool_device_ms = ms.value
        counts, meta = np.zeros((S, n, 4), dtype=np.uint32), np.zeros((S, n), dtype=np.uint8)
        for i in range(S):
            check(self.lib.isx_cmpset_pool_fetch_sample(self.h, i, counts[i].ctypes.data, meta[i].ctypes.data))
        self.pool_raw = {"summary": summary, "counts": counts, "meta": meta}
        gpos = summary["gpos"].astype(np.int64)
        scaf = np.searchsorted(self.offsets, gpos, side="right") - 1
        position = gpos - self.offsets[scaf]
        cats = pd.CategoricalDtype([self.names[i] for i in np.unique(scaf)])
        names = np.array(self.names, dtype=object)
        # DSTdb: one row per (sample that has the scaffold, site)
        si, ri = np.nonzero(meta & _lib.POOL_META_HAS)
        order = np.lexsort((ri, si, scaf[ri]))
        si, ri = si[order], ri[order]
        c = counts[si, ri].astype(np.int64)
        dst = pd.DataFrame({"A": c[:, 0], "C": c[:, 1], "T": c[:, 2], "G": c[:, 3]},
                           index=pd.MultiIndex.from_arrays([np.array(self.samples, dtype=object)[si], position[ri]]))
        dst["scaffold"] = pd.Categorical(names[scaf[ri]], dtype=cats)
        # PMdb
        tot = summary["cnt"].astype(np.int64)
        key = summary["n_con_bases"].astype(np.int64) * 256 + summary["con_bases"]
        text = {k: str(np.array(["ACTG"[(k & 255) >> (2 * j) & 3] for j in range(k >> 8)], dtype=object)) for k in np.unique(key).tolist()}
        pm = pd.DataFrame({"A": tot[:, 0], "C": tot[:, 1], "T": tot[:, 2], "G": tot[:, 3]}, index=position)
        pm["scaffold"] = pd.Categorical(names[scaf], dtype=cats)
        pm["depth"] = tot.sum(axis=1)
        pm["ref_base"] = BASES[np.minimum(summary["ref_base"], 4)]
        pm["sample_5x_detections"] = summary["n_detect_5x"].astype(np.int64)
        pm["sample_detections"] = summary["n_detect"].astype(np.int64)
        for j, cls in enumerate(POOL_CLASSES):
            pm[cls + "_count"] = summary["cls_count"][:, j].astype(np.int64)
        pm["sample_con_bases"] = pd.Series(key, index=pm.index).map(text).astype(object) if n else np.zeros(0, dtype=object)
        pm["con_base"] = BASES[summary["con_base"]]
        pm["var_base"] = BASES[summary["var_base"]]
        return dst, pm

    # ---- strain clustering (compare_utils.py:205-255; include/instrain_amd.h isx_cmpset_cluster) ----
    def strain_clusters(self, stb, bin2length=None, ani_threshold=0.99999, coverage_treshold=0.1, clusterAlg="average", logs=None):
        """-> Cdb (cluster, sample, genome) of the genomes `stb` (scaffold -> genome) makes of the set's scaffolds, from the counters of
        the last compare() (needed since the last add_batch).  bin2length: genome -> length, None = the summed lengths of the genome's
        scaffolds in the set.  A genome with a pair that compared no base (the reference's rule) or with two samples that share no
        scaffold of it (the reference raises there) is left out with a line in `logs`; the others are numbered 1, 2, ... in sorted order."""
        import pandas as pd
        _cluster_method(clusterAlg)
        genome_of = [stb.get(n) for n in self.names]
        genomes = sorted({g for g in genome_of if g is not None})
        self.cluster_genomes, self.cluster_status, self.cluster_labels = genomes, None, None
        if not genomes:                                         # (stb names no scaffold of the set)
            return pd.DataFrame({"cluster": [], "sample": [], "genome": []})
        at = {g: i for i, g in enumerate(genomes)}
        sg = np.array([-1 if g is None else at[g] for g in genome_of], dtype=np.int32)
        if bin2length is None:
            lengths = np.bincount(sg[sg >= 0], weights=self.lengths[sg >= 0], minlength=len(genomes)).astype(np.float64)
        else:
            lengths = np.array([bin2length.get(g, np.nan) for g in genomes], dtype=np.float64)
        S = len(self.samples)
        order = sorted(range(S), key=lambda i: self.samples[i])
        rank = np.zeros(max(S, 1), dtype=np.int32)
        rank[order] = np.arange(S, dtype=np.int32)
        status = np.zeros(len(genomes), dtype=_lib.CLUSTER_STATUS_DT)
        labels = np.zeros((len(genomes), max(S, 1)), dtype=np.int32)
        ms = C.c_float(0)
        check(self.lib.isx_cmpset_cluster(self.h, len(genomes), sg.ctypes.data, lengths.ctypes.data, rank.ctypes.data, clusterAlg.encode(),
                                          1.0 - float(ani_threshold), float(coverage_treshold), status.ctypes.data, labels.ctypes.data,
                                          C.byref(ms)))
        self.cluster_device_ms, self.cluster_status, self.cluster_labels = ms.value, status, labels
        by_rank = labels[:, order]                              # columns in the order of the names
        return _cdb(genomes, status["status"], by_rank, np.array(self.samples, dtype=object)[order], logs)

    def cluster_pairs(self):
        """the genome roll-up of the last strain_clusters(): GENOME_PAIR_DT [genome in .cluster_genomes order, pair as
        itertools.combinations of .samples]"""
        S = len(self.samples)
        out = np.zeros((len(self.cluster_genomes), S * (S - 1) // 2), dtype=_lib.GENOME_PAIR_DT)
        check(self.lib.isx_cmpset_cluster_fetch_pairs(self.h, out.ctypes.data))
        return out

    def cluster_linkage(self, genome):
        """Z (scipy's linkage matrix) of one clustered genome of the last strain_clusters(); points = its samples sorted by name"""
        g = self.cluster_genomes.index(genome)
        Z = np.zeros((max(int(self.cluster_status["n_points"][g]) - 1, 1), 4), dtype=np.float64)
        check(self.lib.isx_cmpset_cluster_fetch_linkage(self.h, g, Z.ctypes.data))
        return Z[:int(self.cluster_status["n_points"][g]) - 1]

    def close(self):
        if self.h:
            self.lib.isx_cmpset_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pool_stored(sset, name2bam, name2r2m=None, max_obs=1 << 24, **filter_flags):
    """pull_SNVS_from_bams (polymorpher.py:102-130) for a pooling SampleSet whose samples came from stored profiles
    (add_profile_pooled) and whose pool_sites() has run.  name2bam: sample -> its .bam.  Per sample: pool_plan(); the BAM is opened and
    scanned once; per planned scaffold its read pairs are name2r2m[sample][scaffold] ({pair: mm} or pair names, through set_r2m) or,
    where that is None / missing, the built-in filter with filter_flags (min_read_ani, min_mapq, max_insert_relative, min_insert,
    pairing_filter) -- the convention of extract_SNVS_from_bam; then the planned columns [lo, hi) go through pool_add_obs() in column
    windows and pool_obs_done() closes the sample.
    The window rule: a scaffold starts with one window of all its hi - lo columns; a window that expands to more than max_obs
    observations is dropped unsent and walked again at the width its own depth allows -- max_obs x columns / observations of the dropped
    window, at most half its width, never below one column (which goes whatever it holds) -- and the rest of the scaffold keeps that
    width.  So host and device staging stay near 8 bytes x max_obs at any depth, no column goes twice
    and none is left out.
    -> {sample: {"scaffolds", "windows", "observations", "device_ms"}}.  A planned scaffold the BAM does not name raises ValueError."""
    from . import engine
    fkw = dict(min_read_ani=filter_flags.get('min_read_ani', 0.95), min_mapq=filter_flags.get('min_mapq', -1),
               max_insert_relative=filter_flags.get('max_insert_relative', 3), min_insert=filter_flags.get('min_insert', 50),
               pairing_filter=filter_flags.get('pairing_filter', 'paired_only'))
    out = {}
    for name, bam in name2bam.items():
        plan = sset.pool_plan(name)
        stats = {"scaffolds": len(plan), "windows": 0, "observations": 0, "device_ms": 0.0}
        bf = engine.BamFile(bam)
        try:
            tid = {n: i for i, (n, _, _) in enumerate(bf.refs())}
            for scaffold in plan:
                if scaffold not in tid:
                    raise ValueError("scaffold {0} is not in the .bam file {1}!".format(scaffold, bam))
            bf.scan()
            r2m = {s: (name2r2m or {}).get(name, {}).get(s) for s in plan}
            if any(m is None for m in r2m.values()):
                bf.filter(**fkw)
            for scaffold, m in r2m.items():
                if m is not None:
                    bf.set_r2m(tid[scaffold], list(m), None)
            for scaffold, (lo, hi, _) in plan.items():
                a, width = lo, hi - lo
                while a < hi:
                    b = min(a + width, hi)
                    obs, _, _, _ = bf.expand_region(tid[scaffold], a, b, skip_mm=True, copy=False, **fkw)
                    if len(obs) > max_obs and b - a > 1:           # the width the dropped window's depth allows, at most half
                        width = max(1, min((b - a + 1) // 2, int(max_obs * (b - a) // len(obs))))
                        continue
                    stats["device_ms"] += sset.pool_add_obs(name, [scaffold], obs, [0, len(obs)])
                    stats["windows"] += 1
                    stats["observations"] += int(len(obs))
                    a = b
            sset.pool_obs_done(name, list(plan))
        finally:
            bf.close()
        out[name] = stats
    return out


def genome_wide(table, stb, bin2length=None, mm_level=False):
    """genomeUtilities._genome_wide_readComparer (genomeUtilities.py:739-800) on _add_stb(table, stb) (:430-448): the scaffold-level
    comparison rows rolled up per (genome, name1, name2) -- per mm when mm_level, else from every scaffold's highest-mm row.
    table: compare()'s rows (or a DataFrame of them); stb: scaffold -> genome; scaffolds it does not name are left out.
    -> DataFrame with the reference's columns and row order, None when there is no row / no genome (as _add_stb)."""
    import pandas as pd
    gdb = table.copy() if isinstance(table, pd.DataFrame) else pd.DataFrame(list(table))
    if len(gdb) == 0:
        return None
    gdb["genome"] = gdb["scaffold"].map(stb)
    if gdb["genome"].notna().sum() == 0:
        return None
    key = ["scaffold", "name1", "name2"]
    gdb = gdb.sort_values("mm", kind="stable")
    if not mm_level:
        gdb = gdb.drop_duplicates(subset=key, keep="last").copy()
        gdb["mm"] = 0
    n = gdb["compared_bases_count"].astype(np.float64)
    gdb["_w_overlap"] = gdb["coverage_overlap"].astype(np.float64) * n
    ani = [c for c in ("ANI", "popANI", "conANI") if c in gdb.columns]
    for c in ani:                                   # a NaN ANI (nothing compared on the scaffold) counts as 0 (:788)
        v = gdb[c].astype(np.float64)
        gdb["_w_" + c] = np.where(v == v, v * n, 0.0)
    sums = [c for c in ("compared_bases_count", "consensus_SNPs", "population_SNPs") if c in gdb.columns]
    parts = []
    for mm in sorted(gdb["mm"].unique()):
        odb = gdb[gdb["mm"] <= mm].drop_duplicates(subset=key, keep="last")
        g = odb.groupby(["genome", "name1", "name2"], sort=True)[sums + ["_w_overlap"] + ["_w_" + c for c in ani]].sum().reset_index()
        tcb = g["compared_bases_count"]
        some = (tcb != 0).to_numpy()
        d = {"genome": g["genome"], "name1": g["name1"], "name2": g["name2"], "mm": mm}
        with np.errstate(divide="ignore", invalid="ignore"):
            d["coverage_overlap"] = np.where(some, g["_w_overlap"].to_numpy() / tcb.to_numpy(), np.nan)
            for c in sums:
                d[c] = g[c]
            for c in ani:
                d[c] = np.where(some, g["_w_" + c].to_numpy() / tcb.to_numpy(), np.nan)
            if bin2length is not None:
                d["percent_compared"] = tcb.to_numpy() / g["genome"].map(bin2length).to_numpy(dtype=np.float64)
        parts.append(pd.DataFrame(d))
    db = pd.concat(parts, ignore_index=True)
    if not mm_level:
        del db["mm"]
    return db


# ---- strain clustering (compare_utils.py:169-284) ----
def _cluster_method(name):
    if name not in _lib.CLUSTER_METHODS:
        raise ValueError("clusterAlg %r is not supported: %s are (scipy runs other algorithms than the NN-chain for single, centroid, "
                         "median and ward)" % (name, ", ".join(_lib.CLUSTER_METHODS)))
    return name.encode()


def cluster_skip_line(genome, status):
    """the log line of a genome that is not clustered"""
    if status == _lib.CLUSTER_NO_OVERLAP:                       # (the reference's line, compare_utils.py:263, without its counts)
        return "Cannot cluster genome %s; some comparisons involve no genomic overlap at all" % (genome,)
    return "Cannot cluster genome %s; some pair of its samples was never compared (not every pair shares a scaffold of it)" % (genome,)


def _cdb(genomes, status, labels, names, logs):
    """genomes sorted, status[genome], labels[genome, sample by name] (0 = not a member), names sorted -> Cdb"""
    import pandas as pd
    status = np.asarray(status)
    if logs is not None:
        for g in np.flatnonzero((status == _lib.CLUSTER_NO_OVERLAP) | (status == _lib.CLUSTER_MISSING_PAIR)):
            logs.append(cluster_skip_line(genomes[g], int(status[g])))
    number = np.cumsum(status == _lib.CLUSTER_OK)               # the genomes actually clustered count from 1
    lab = np.where((status == _lib.CLUSTER_OK)[:, None], labels, 0)
    gi, si = np.nonzero(lab)
    cluster = np.char.add(np.char.add(number[gi].astype(str), "_"), lab[gi, si].astype(str)).astype(object) if len(gi) else np.zeros(0, object)
    return pd.DataFrame({"cluster": cluster, "sample": np.asarray(names, dtype=object)[si], "genome": np.asarray(genomes, dtype=object)[gi]})


def _linkage_batch(ctx, n_points, offsets, values, method, cutoff, want_Z=True):
    """isx_cluster_linkage -> (labels of problem 0, 1, ... in one array, Z rows or None, device ms)"""
    n_points = np.ascontiguousarray(n_points, dtype=np.int32)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    values = np.ascontiguousarray(values, dtype=np.float64)
    n_pts = int(n_points.astype(np.int64).sum())
    labels = np.zeros(max(n_pts, 1), dtype=np.int32)
    Z = np.zeros((max(n_pts - len(n_points), 1), 4), dtype=np.float64) if want_Z else None
    ms = C.c_float(0)
    check(ctx.lib.isx_cluster_linkage(ctx.h, len(n_points), n_points.ctypes.data, offsets.ctypes.data, values.ctypes.data, len(values),
                                      method if isinstance(method, bytes) else str(method).encode(), float(cutoff), labels.ctypes.data,
                                      None if Z is None else Z.ctypes.data, C.byref(ms)))
    return labels[:n_pts], (None if Z is None else Z[:n_pts - len(n_points)]), ms.value


def linkage_flat(ctx, matrices, method, cutoff):
    """scipy.cluster.hierarchy.linkage(m, method) + fcluster(Z, cutoff, criterion='distance') for a batch of distance matrices (square
    and symmetric with a zero diagonal, or condensed) on the device -> [(labels int32[n], Z float64[n - 1, 4])], bit-equal to scipy's"""
    _cluster_method(method)
    cond, n_points = [], []
    for k, m in enumerate(matrices):
        m = np.asarray(m, dtype=np.float64)
        if m.ndim == 2:
            if m.shape[0] != m.shape[1] or not (np.array_equal(m, m.T, equal_nan=True) and (np.diagonal(m) == 0).all()):
                raise ValueError("linkage_flat: matrix %d is not square and symmetric with a zero diagonal" % k)
            n = m.shape[0]
            m = m[np.triu_indices(n, 1)]
        elif m.ndim == 1:
            n = int(round((1 + np.sqrt(1 + 8 * len(m))) / 2))
            if n * (n - 1) // 2 != len(m):
                raise ValueError("linkage_flat: %d values are no condensed distance matrix (matrix %d)" % (len(m), k))
        else:
            raise ValueError("linkage_flat: matrix %d has %d dimensions" % (k, m.ndim))
        cond.append(m)
        n_points.append(n)
    if not cond:
        return []
    offsets = np.r_[0, np.cumsum([len(c) for c in cond])][:-1]
    labels, Z, _ = _linkage_batch(ctx, n_points, offsets, np.concatenate(cond), method, cutoff)
    p0 = np.r_[0, np.cumsum(n_points)]
    return [(labels[p0[k]:p0[k + 1]].copy(), Z[p0[k] - k:p0[k + 1] - k - 1].copy()) for k in range(len(cond))]


def cluster_genome_strains(ctx, Mdb, ani_threshold=0.99999, coverage_treshold=0.1, clusterAlg="average", logs=None, details=None):
    """compare_utils.cluster_genome_strains (compare_utils.py:205-255) on a genome_wide() / stored genomeWide_compare frame (columns genome,
    name1, name2, compared_bases_count, popANI, percent_compared) -> Cdb (cluster, sample, genome).  The matrices are made here by
    numpy / pandas, every genome's linkage and flat clusters on the device (isx_cluster_linkage) in one call.  Genomes that cannot be
    clustered are left out with a line in `logs` (see SampleSet.strain_clusters).  details: a dict that receives genomes, status,
    samples, matrices (condensed), Z and device_ms of the call."""
    import pandas as pd
    method = _cluster_method(clusterAlg)
    for c in ("genome", "name1", "name2", "compared_bases_count", "popANI", "percent_compared"):
        if c not in Mdb.columns:
            raise ValueError("cluster_genome_strains: the table has no column %r (genome_wide needs bin2length for percent_compared)" % c)
    db = Mdb[Mdb["name1"] != Mdb["name2"]]
    gcode, genomes = pd.factorize(db["genome"], sort=True)
    G = len(genomes)
    # rule 2: a genome's samples, sorted by name
    pts = pd.DataFrame({"g": np.r_[gcode, gcode], "s": np.r_[db["name1"].to_numpy(dtype=object), db["name2"].to_numpy(dtype=object)]})
    pts = pts.drop_duplicates().sort_values(["g", "s"], kind="stable").reset_index(drop=True)
    n_of = np.bincount(pts["g"].to_numpy(), minlength=G).astype(np.int64)
    pt_off = np.r_[0, np.cumsum(n_of)]
    where = pd.MultiIndex.from_arrays([pts["g"], pts["s"]])
    a = where.get_indexer(pd.MultiIndex.from_arrays([gcode, db["name1"].to_numpy(dtype=object)])) - pt_off[gcode]
    b = where.get_indexer(pd.MultiIndex.from_arrays([gcode, db["name2"].to_numpy(dtype=object)])) - pt_off[gcode]
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    # rules 3, 4
    n_val = n_of * (n_of - 1) // 2
    val_off = np.r_[0, np.cumsum(n_val)]
    values = np.full(int(val_off[-1]), np.nan)
    pc = db["percent_compared"].to_numpy(dtype=np.float64)
    with np.errstate(invalid="ignore"):
        dist = np.where(pc < coverage_treshold, 1.0, 1.0 - db["popANI"].to_numpy(dtype=np.float64))
    values[val_off[gcode] + n_of[gcode] * lo - lo * (lo + 1) // 2 + (hi - lo - 1)] = dist
    status = np.full(G, _lib.CLUSTER_OK, dtype=np.int32)
    holes = np.add.reduceat(np.r_[np.isnan(values), False].astype(np.int64), val_off[:-1])[:G] if G else np.zeros(0, np.int64)
    status[(holes > 0) & (n_val > 0)] = _lib.CLUSTER_MISSING_PAIR
    status[np.bincount(gcode, weights=(db["compared_bases_count"].to_numpy() == 0), minlength=G) > 0] = _lib.CLUSTER_NO_OVERLAP
    ok = np.flatnonzero(status == _lib.CLUSTER_OK)
    S_all = pts["s"].to_numpy(dtype=object)
    names = sorted(set(S_all.tolist()))
    col = pd.Index(names).get_indexer(S_all)
    labels = np.zeros((G, max(len(names), 1)), dtype=np.int32)
    Z, ms = None, 0.0
    if len(ok):
        keep = np.repeat(status == _lib.CLUSTER_OK, n_of)
        flat, Z, ms = _linkage_batch(ctx, n_of[ok], val_off[ok], values, method, 1.0 - float(ani_threshold))
        labels[pts["g"].to_numpy()[keep], col[keep]] = flat
    if details is not None:
        z0 = np.r_[0, np.cumsum(n_of[ok] - 1)]
        details.update(genomes=list(genomes), status=status, device_ms=ms,
                       samples={genomes[g]: S_all[pt_off[g]:pt_off[g + 1]].tolist() for g in range(G)},
                       matrices={genomes[g]: values[val_off[g]:val_off[g + 1]].copy() for g in range(G)},
                       Z={genomes[g]: Z[z0[k]:z0[k + 1]].copy() for k, g in enumerate(ok)})
    return _cdb(list(genomes), status, labels, names, logs)


# ---- the user tables of SNV pooling (SNVprofile.py:367-410) ----
POOLED_SNV_INFO_COLUMNS = ["scaffold", "position", "depth", "A", "C", "T", "G", "ref_base", "con_base", "var_base", "sample_detections",
                           "sample_5x_detections", "DivergentSite_count", "SNS_count", "SNV_count", "con_SNV_count", "pop_SNV_count"]


def pooled_SNV_info(PMdb):
    """pooled_SNV_info (SNVprofile.py:367-375): PMdb with `position` as a column, the reference's column order, whatever else PMdb
    holds (sample_con_bases) behind it"""
    db = PMdb.copy()
    db["position"] = db.index
    db = db.reset_index(drop=True)
    if len(db) == 0:
        return db
    return db[[c for c in POOLED_SNV_INFO_COLUMNS if c in db.columns] + [c for c in db.columns if c not in POOLED_SNV_INFO_COLUMNS]]


def pooled_SNV_data(DSTdb, samples=None):
    """pooled_SNV_data and pooled_SNV_data_keys (SNVprofile.py:377-410) -> (data: sample, scaffold, position, A, C, T, G with samples and
    scaffolds as integer keys; keys: key, sample, scaffold with NaN where a key names only one of them).  The reference numbers both by
    enumerating a set(); here scaffolds are numbered in category order (the set's) and samples in the order of `samples` (a
    SampleSet's .samples), None = DSTdb's order of first appearance."""
    import pandas as pd
    level0 = DSTdb.index.get_level_values(0)
    if samples is None:
        sample_codes, samples = pd.factorize(level0, sort=False)
    else:
        samples = [s for s in samples if s in set(level0)]
        sample_codes = pd.Index(samples).get_indexer(level0)
    scaffolds = list(DSTdb["scaffold"].cat.categories)
    data = pd.DataFrame({"sample": sample_codes.astype(np.int64), "scaffold": DSTdb["scaffold"].cat.codes.to_numpy().astype(np.int64),
                         "position": DSTdb.index.get_level_values(1).to_numpy().astype(np.int64)})
    for c in "ACTG":
        data[c] = DSTdb[c].to_numpy()
    n = max(len(samples), len(scaffolds))
    keys = pd.DataFrame({"key": np.arange(n),
                         "sample": [samples[i] if i < len(samples) else np.nan for i in range(n)],
                         "scaffold": [scaffolds[i] if i < len(scaffolds) else np.nan for i in range(n)]})
    return data, keys
