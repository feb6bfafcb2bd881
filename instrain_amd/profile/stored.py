"""A stored profile as the device's third level source (include/instrain_amd.h isx_stored_*): host packing and the files.

The reference keeps a profile's covT / clonT / clonTR as raw_data/*.hd5 (SNVprofile._store_special, SNVprofile.py:717-733) and
its tables as raw_data/*.csv.gz; `inStrain profile_genes -i IS` (GeneProfile.calculate_gene_metrics) and `inStrain genome_wide
-i IS` (genomeUtilities.genomeLevel_from_IS) start from them.  pack_levels lays the series of some scaffolds out the way
isx_stored_create takes them -- numpy only, no device; store_profile / load_profile write and read the folder;
scaffold_table recomputes the cumulative_scaffold_table from the stored series on the device.
"""
import json
import os

import numpy as np
import pandas as pd

from .. import _lib
from ..compare import SNV_OLD_NAMES, _scaffold_profiles, _series, _whole
from . import emitters

TABLES = ("cumulative_snv_table", "raw_linkage_table", "cumulative_scaffold_table")
SPECIALS = (("covT", "coverage"), ("clonT", "clonality"), ("clonTR", "clonality"))


def _cov_series(ser, what, length):
    try:
        return _series(ser, what, length)
    except ValueError as e:
        raise ValueError(str(e).replace("pack_profile:", "pack_levels:"))


def _clon_series(ser, what, length):
    """one clonT / clonTR series -> (ascending uint32 positions, float32 values in (0, 1])"""
    pos, val = ser if isinstance(ser, tuple) else (ser.index.to_numpy(), ser.to_numpy())
    try:
        pos = _whole(pos, what + " positions", length - 1)
    except ValueError as e:
        raise ValueError(str(e).replace("pack_profile:", "pack_levels:"))
    val = np.asarray(val)
    if val.dtype.kind not in "fiu":
        raise ValueError("pack_levels: %s values are not numeric (%s)" % (what, val.dtype))
    val = val.astype(np.float32)
    if pos.shape != val.shape or pos.ndim != 1:
        raise ValueError("pack_levels: %s has not one value per position" % what)
    if not (np.isfinite(val) & (val > 0) & (val <= 1)).all():
        raise ValueError("pack_levels: %s holds a clonality that is NaN or outside (0, 1]" % what)
    if len(pos) > 1 and (pos[1:] <= pos[:-1]).any():
        order = np.argsort(pos, kind="stable")
        pos, val = pos[order], val[order]
        if (pos[1:] == pos[:-1]).any():
            raise ValueError("pack_levels: %s names a position twice" % what)
    return pos.astype(np.uint32), val


def table_levels(tables, scaffolds=None):
    """the sorted union of the mm keys of {scaffold: {mm: series}} tables (None entries are skipped) over `scaffolds` (None: all)"""
    keys = set()
    for t in tables:
        for n, d in (t or {}).items():
            if scaffolds is None or n in scaffolds:
                keys.update(int(mm) for mm in d)
    return sorted(keys)


def pack_levels(scaffolds, lengths, covT, clonT=None, clonTR=None, mm_values=None):
    """The series of `scaffolds` (names; `lengths` their lengths) as the arrays of isx_stored_create.  covT / clonT / clonTR:
    {scaffold: {mm: pd.Series(values, index=positions)}} (emitters.load_special) or (positions, values) tuples in place of a Series.
    -> {"scaffolds", "bounds" int64 [n + 1], "levels" int32 (strictly ascending: the sorted union of the three tables' keys over these
    scaffolds, or mm_values), "cov_present" / "clon_present" uint8 [n, n_levels] (the level is a key of the scaffold's covT / clonT,
    whether or not its series is empty) and per table a LEVEL-MAJOR CSR: "cov_offsets" / "clon_offsets" / "clonr_offsets" int64
    [n_levels + 1], "*_gpos" uint32 flat positions, "cov_values" uint32 / "clon_values", "clonr_values" float32}.  Inside a level the
    entries lie scaffold after scaffold and ascend within one, so a level is one slice ordered by flat position.  A scaffold no table
    names stays in the flat space with nothing on it (the reference profiles "no reads" as zeros).  A series whose index does not
    ascend is sorted.  ValueError, naming the series: a position twice or beyond the scaffold, a fractional / negative / NaN
    coverage, a clonality that is NaN or outside (0, 1]; also a key that mm_values does not name."""
    scaffolds = list(scaffolds)
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if len(lengths) != len(scaffolds) or (lengths <= 0).any():
        raise ValueError("pack_levels: one positive length per scaffold")
    bounds = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    if bounds[-1] > 0xFFFFFFFF:
        raise ValueError("pack_levels: %d positions, a flat space holds fewer than 2^32 (pack fewer scaffolds)" % bounds[-1])
    sources = [("covT", covT or {}, _cov_series, np.uint32), ("clonT", clonT or {}, _clon_series, np.float32),
               ("clonTR", clonTR or {}, _clon_series, np.float32)]
    keyed = [{n: {int(mm): ser for mm, ser in t.get(n, {}).items()} for n in scaffolds} for _, t, _, _ in sources]
    union = sorted({mm for k in keyed for d in k.values() for mm in d})
    if mm_values is None:
        levels = np.array(union, dtype=np.int32)
    else:
        levels = np.array(mm_values, dtype=np.int32).reshape(-1)
        if len(levels) > 1 and (levels[1:] <= levels[:-1]).any():
            raise ValueError("pack_levels: mm_values must ascend strictly")
        missing = sorted(set(union) - set(levels.tolist()))
        if missing:
            raise ValueError("pack_levels: the tables have the keys %s, which mm_values does not name" % missing)
    L = len(levels)
    out = {"scaffolds": scaffolds, "bounds": bounds, "levels": levels}
    for (name, _, read, dtype), keys, short in zip(sources, keyed, ("cov", "clon", "clonr")):
        present = np.zeros((len(scaffolds), L), dtype=np.uint8)
        offsets = np.zeros(L + 1, dtype=np.int64)
        pos_parts, val_parts = [np.zeros(0, np.uint32)], [np.zeros(0, dtype)]
        for k, mm in enumerate(levels.tolist()):
            n_here = 0
            for i, n in enumerate(scaffolds):
                if mm not in keys[n]:
                    continue
                present[i, k] = 1
                p, v = read(keys[n][mm], "%s[%r][%d]" % (name, n, mm), int(lengths[i]))
                pos_parts.append((p.astype(np.int64) + bounds[i]).astype(np.uint32))
                val_parts.append(v.astype(dtype))
                n_here += len(p)
            offsets[k + 1] = offsets[k] + n_here
        out[short + "_offsets"], out[short + "_gpos"], out[short + "_values"] = offsets, np.concatenate(pos_parts), np.concatenate(val_parts)
        if short != "clonr":
            out[short + "_present"] = present
    return out


# ---- the folder ----
def store_profile(folder, profiles, scaffold2length=None):
    """covT.hd5, clonT.hd5, clonTR.hd5, cumulative_snv_table.csv.gz, raw_linkage_table.csv.gz and cumulative_scaffold_table.csv.gz of a
    sample under `folder`, under the reference's attribute names and in its formats (profile.emitters); scaffold2length (name ->
    length) also as scaffold2length.json, one JSON object, the way the reference stores an attribute of type 'dictionary'.
    profiles: the sample's scaffold profiles (scaffold_profile.from_splits), or what profile_bam returns.  -> {name: path}"""
    profs = _scaffold_profiles(profiles)
    os.makedirs(folder, exist_ok=True)
    out = {}
    for name, _ in SPECIALS:
        out[name] = emitters.store_special({P.scaffold: getattr(P, name) for P in profs if getattr(P, name, None)}, os.path.join(folder, name))
    for name in TABLES:
        parts = [getattr(P, name) for P in profs if getattr(P, name, None) is not None and len(getattr(P, name))]
        out[name] = emitters.store_pandas(pd.concat(parts).reset_index(drop=True) if parts else pd.DataFrame(), os.path.join(folder, name))
    if scaffold2length is not None:
        out["scaffold2length"] = os.path.join(folder, "scaffold2length.json")
        with open(out["scaffold2length"], "w") as fp:
            json.dump({str(k): int(v) for k, v in dict(scaffold2length).items()}, fp)
    return out


def load_profile(folder, scaffolds=None):
    """-> {"covT", "clonT", "clonTR": {scaffold: {mm: pd.Series}}, "cumulative_snv_table", "raw_linkage_table",
    "cumulative_scaffold_table": DataFrames, "scaffold2length": dict when the folder has it} of a folder store_profile wrote, or of the
    raw_data folder of a profile the reference wrote.  A file that is not there gives an empty dict / frame.  scaffolds: load only these."""
    want = None if scaffolds is None else set(scaffolds)
    out = {}
    for name, kind in SPECIALS:
        path = os.path.join(folder, name + ".hd5")
        out[name] = emitters.load_special(path, kind=kind, scaffolds=want) if os.path.exists(path) else {}
    for name in TABLES:
        path = os.path.join(folder, name + ".csv.gz")
        try:
            db = pd.read_csv(path, index_col=0, float_precision="round_trip") if os.path.exists(path) else pd.DataFrame()
        except pd.errors.EmptyDataError:
            db = pd.DataFrame()
        if want is not None and "scaffold" in db.columns:
            db = db[db["scaffold"].isin(want)].reset_index(drop=True)
        out[name] = db
    path = os.path.join(folder, "scaffold2length.json")
    if os.path.exists(path):
        with open(path, "r") as fp:
            s2l = {k: int(v) for k, v in json.load(fp).items()}
        out["scaffold2length"] = s2l if want is None else {k: v for k, v in s2l.items() if k in want}
    return out


# ---- the stored tables as device rows ----
def chunk_scaffolds(names, lengths, max_positions):
    """whole scaffolds in order, at most max_positions flat positions a chunk; a longer scaffold goes alone -> lists of indices"""
    chunks, cur, size = [], [], 0
    for i, ln in enumerate(lengths):
        if cur and size + int(ln) > int(max_positions):
            chunks.append(cur)
            cur, size = [], 0
        cur.append(i)
        size += int(ln)
    if cur:
        chunks.append(cur)
    return chunks


def _level_rank(mm, levels, what):
    mm = np.asarray(mm, dtype=np.int64)
    levels = np.asarray(levels, dtype=np.int64)
    rank = np.searchsorted(levels, mm)
    bad = (rank >= len(levels)) | (levels[np.minimum(rank, len(levels) - 1)] != mm)
    if bad.any():
        raise ValueError("%s has rows at mm %s, which is no level of the profile's covT" % (what, sorted(set(mm[bad].tolist()))))
    return rank


_BASE_CODE = {"A": 0, "C": 1, "T": 2, "G": 3}


def snv_rows(snv_table, offsets, levels):
    """the rows of a stored cumulative_snv_table on the scaffolds of `offsets` (name -> flat offset) as SNV_DT rows in (gpos, mm)
    order: mm = the rank of the row's mm in `levels`, cls = the isx_snv.cls code of its class (snv_utilities.CLASSES)"""
    from .snv_utilities import CLASSES
    if snv_table is None or len(snv_table) == 0:
        return np.zeros(0, dtype=_lib.SNV_DT)
    db = snv_table.rename(columns=SNV_OLD_NAMES)
    db = db[db["scaffold"].astype(object).isin(set(offsets))]
    if len(db) == 0:
        return np.zeros(0, dtype=_lib.SNV_DT)
    for col in ("position", "mm", "allele_count", "class"):
        if col not in db.columns:
            raise ValueError("the stored SNV table has no column %s" % col)
    gpos = db["scaffold"].astype(object).map(offsets).to_numpy(np.int64) + _whole(db["position"].to_numpy(), "SNV positions", 0xFFFFFFFF)
    rank = _level_rank(_whole(db["mm"].to_numpy(), "SNV mm", 65535), levels, "the stored SNV table")
    code = np.array([CLASSES.index(c) if c in CLASSES else -1 for c in db["class"].astype(object)], dtype=np.int64)
    if (code < 0).any():
        raise ValueError("the stored SNV table's column class holds %r" % sorted({str(c) for c, k in zip(db["class"].astype(object), code) if k < 0}))
    order = np.lexsort((rank, gpos))
    v = np.zeros(len(db), dtype=_lib.SNV_DT)
    v["gpos"], v["mm"], v["cls"] = gpos[order], rank[order], code[order]
    v["allele_count"] = np.clip(_whole(db["allele_count"].to_numpy(), "allele_count", 1 << 30)[order], 0, 255)
    for col in ("con_base", "var_base", "ref_base"):
        if col in db.columns:
            v[col] = [_BASE_CODE.get(b, 4) for b in db[col].astype(object).to_numpy()[order]]
    for j, b in enumerate("ACTG"):
        if b in db.columns:
            v["cnt"][:, j] = _whole(db[b].to_numpy(), "the SNV table's column " + b, 0xFFFFFFFF)[order]
    if "cryptic" in db.columns:
        v["cryptic"] = db["cryptic"].to_numpy().astype(bool)[order]
    return v


def ld_rows(linkage_table, offsets, levels):
    """the rows of a stored raw_linkage_table on the scaffolds of `offsets` as LD_DT rows in (gpos_a, gpos_b, mm) order, mm as in snv_rows"""
    if linkage_table is None or len(linkage_table) == 0:
        return np.zeros(0, dtype=_lib.LD_DT)
    db = linkage_table[linkage_table["scaffold"].astype(object).isin(set(offsets))]
    if len(db) == 0:
        return np.zeros(0, dtype=_lib.LD_DT)
    off = db["scaffold"].astype(object).map(offsets).to_numpy(np.int64)
    ga = off + _whole(db["position_A"].to_numpy(), "linkage position_A", 0xFFFFFFFF)
    gb = off + _whole(db["position_B"].to_numpy(), "linkage position_B", 0xFFFFFFFF)
    rank = _level_rank(_whole(db["mm"].to_numpy(), "linkage mm", 65535), levels, "the stored linkage table")
    order = np.lexsort((rank, gb, ga))
    v = np.zeros(len(db), dtype=_lib.LD_DT)
    v["gpos_a"], v["gpos_b"], v["mm"] = ga[order], gb[order], rank[order]
    for col in ("r2", "d_prime", "r2_normalized", "d_prime_normalized"):
        v[col] = db[col].to_numpy(np.float64)[order] if col in db.columns else np.nan
    for col in ("total", "countAB", "countAb", "countaB", "countab"):
        if col in db.columns:
            v[col] = _whole(db[col].to_numpy(), "linkage " + col, 0xFFFFFFFF)[order]
    return v


def profile_levels(profile):
    """the levels of a loaded profile: the sorted union of the keys of its covT / clonT / clonTR ([0] for a profile without any)"""
    return table_levels([profile.get("covT"), profile.get("clonT"), profile.get("clonTR")]) or [0]


def level_chunks(ctx, profile, names, lengths, levels, max_positions=1 << 27, ref_of=None):
    """chunk after chunk of whole scaffolds (chunk_scaffolds): (names, lengths, pack, engine.StoredLevels) -- the object is closed when
    the generator moves on.  ref_of: None, or name -> base codes of the scaffold (uint8, engine.encode_seq)"""
    from .. import engine
    for idx in chunk_scaffolds(names, lengths, max_positions):
        cn, cl = [names[i] for i in idx], [int(lengths[i]) for i in idx]
        pack = pack_levels(cn, cl, profile.get("covT"), profile.get("clonT"), profile.get("clonTR"), mm_values=levels)
        ref = None if ref_of is None else np.concatenate([np.asarray(ref_of(n), dtype=np.uint8) for n in cn])
        st = engine.StoredLevels(ctx, pack, ref_codes=ref)
        try:
            yield cn, cl, pack, st
        finally:
            st.close()


def scaffold_table(ctx, profile, scaffold2length, scaffolds=None, max_positions=1 << 27):
    """{scaffold: cumulative_scaffold_table} recomputed from a loaded profile's series: StoredLevels.summarize and
    engine.snv_level_counts on the stored SNV table, through profile_utilities.make_coverage_table -- what profile_bam(scaffold_tables=)
    fills.  scaffolds: None = every scaffold of scaffold2length that covT names"""
    from .. import engine
    from .profile_utilities import make_coverage_table
    covT = profile.get("covT") or {}
    names = [n for n in scaffold2length if n in covT] if scaffolds is None else list(scaffolds)
    levels = profile_levels(profile)
    out = {}
    for cn, cl, pack, st in level_chunks(ctx, profile, names, [scaffold2length[n] for n in names], levels, max_positions):
        rows, _ = st.summarize()
        rows["mm"] = np.asarray(levels, dtype=np.int64)[rows["mm"].astype(np.int64)]
        offsets = dict(zip(cn, pack["bounds"][:-1].tolist()))
        counts, _ = engine.snv_level_counts(ctx, snv_rows(profile.get("cumulative_snv_table"), offsets, levels), pack["bounds"], len(levels))
        for j, n in enumerate(cn):
            out[n] = make_coverage_table(rows[j], cl[j], n, None, counts[j])
    return out
