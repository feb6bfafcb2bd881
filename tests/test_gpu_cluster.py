"""GPU: strain clustering on the device (instrain_amd/csrc/isx_cluster.hip through compare.linkage_flat, compare.cluster_genome_strains
and SampleSet.strain_clusters) against the reference's vectors (tests/golden/make_cluster_golden.py) and, bit for bit, against the numpy
restatement (tests/cluster_ref.py).  Sizes sit on the kernel's edges: one wave (64 points), the LDS matrix (CLUSTER_LDS_MAX_POINTS)."""
import ctypes as C
import itertools
import re

import numpy as np
import pytest

from tests import cluster_ref as cr
from tests import util
from tests.test_cluster_ref import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from instrain_amd import engine
    c = engine.Context(0)
    lut, fb = util.load_lut()
    c.set_null_model(lut, fb)
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden():
    return load_golden()


# ---- 1. the reference's vectors through cluster_genome_strains ----
@pytest.mark.parametrize("method", cr.METHODS)
def test_reference_tables_exactly(ctx, golden, method):
    from instrain_amd import compare
    g = golden
    for t in g["thresholds"]:
        logs, det = [], {}
        cdb = compare.cluster_genome_strains(ctx, g["mdb"], ani_threshold=t, coverage_treshold=g["coverage_treshold"], clusterAlg=method,
                                             logs=logs, details=det)
        assert list(cdb.columns) == ["cluster", "sample", "genome"]
        assert cdb.values.tolist() == g["cdb"]["%s %r" % (method, t)], (method, t)
        assert len(logs) == 1 and logs[0].startswith("Cannot cluster genome gD_zero")
        assert det["device_ms"] > 0
        for genome, e in g["genomes"].items():
            n, ref = len(e["samples"]), np.array(e["Z"][method], dtype=np.float64)
            Z = det["Z"][genome]
            assert det["samples"][genome] == e["samples"]
            assert np.array_equal(Z[:, [0, 1, 3]], ref[:, [0, 1, 3]]) and np.abs(Z[:, 2] - ref[:, 2]).max() <= g["tol"], (genome, method)
            assert Z.tobytes() == cr.linkage(det["matrices"][genome], n, method).tobytes(), (genome, method)


# ---- 2. linkage_flat against the restatement, bit for bit ----
def seeded_matrices():
    """condensed matrices on the kernel's edges: the wave edge, the LDS edge, ties only"""
    from instrain_amd import _lib
    lds = _lib.CLUSTER_LDS_MAX_POINTS
    rng = np.random.Generator(np.random.PCG64(2024))
    out = []
    for n in (2, 3, 63, 64, 65, lds - 1, lds, lds + 1):
        out.append(rng.choice([0.0, 1e-6, 2e-5, 3e-4, 1.0], size=n * (n - 1) // 2))
    for n in (5, 65, lds + 1):
        out.append(rng.random(n * (n - 1) // 2))
    out.append(np.zeros(65 * 64 // 2))                           # all zero
    out.append(np.ones(33 * 32 // 2))                            # all one
    block = np.ones((70, 70))                                    # blocks of zeros: three strains, samples interleaved
    strain = np.arange(70) % 3
    block[strain[:, None] == strain[None, :]] = 0.0
    out.append(block[np.triu_indices(70, 1)])
    out.append(rng.choice([0.0, 1.0], size=12 * 11 // 2))
    return out


CUTOFF = 1.0 - 0.99999


@pytest.fixture(scope="module")
def expected():
    """the restatement's (labels, Z) of every seeded matrix and method, computed once"""
    mats = seeded_matrices()
    return mats, {m: [cr.linkage_flat(v, m, CUTOFF) for v in mats] for m in cr.METHODS}


@pytest.mark.parametrize("method", cr.METHODS)
def test_linkage_flat_equals_the_restatement_bit_for_bit(ctx, expected, method):
    from instrain_amd import compare
    mats, exp = expected
    got = compare.linkage_flat(ctx, mats, method, CUTOFF)        # problems of every size class mixed in one call
    again = compare.linkage_flat(ctx, mats, method, CUTOFF)
    assert len(got) == len(mats)
    for k, ((lab, Z), (elab, eZ)) in enumerate(zip(got, exp[method])):
        n = len(elab)
        assert lab.dtype == np.int32 and Z.shape == (n - 1, 4)
        assert lab.tolist() == elab.tolist(), (k, n, method)
        assert Z.tobytes() == eZ.tobytes(), (k, n, method)
        assert lab.tobytes() == again[k][0].tobytes() and Z.tobytes() == again[k][1].tobytes()      # two calls: identical bytes
    # alone (its own launch) a problem gives what it gave among the others; a square matrix is taken like its condensed form
    for k in (0, 4, len(mats) - 1):
        n = len(exp[method][k][0])
        sq = np.zeros((n, n))
        sq[np.triu_indices(n, 1)] = mats[k]
        (lab, Z), = compare.linkage_flat(ctx, [sq + sq.T], method, CUTOFF)
        assert lab.tobytes() == got[k][0].tobytes() and Z.tobytes() == got[k][1].tobytes()
    assert len({tuple(lab.tolist()) for lab, _ in got}) > 5      # not vacuous: the matrices cluster differently


def test_cutoffs_between_the_heights(ctx, expected):
    """fcluster at other cutoffs than the default one, the all-in-one and the all-apart ends included"""
    from instrain_amd import compare
    mats, _ = expected
    some = [mats[1], mats[4], mats[8], mats[-1]]
    for cutoff in (0.0, 2e-5, 0.5, 1.0):
        for (lab, Z), v in zip(compare.linkage_flat(ctx, some, "average", cutoff), some):
            elab, eZ = cr.linkage_flat(v, "average", cutoff)
            assert lab.tolist() == elab.tolist() and Z.tobytes() == eZ.tobytes()


# ---- 3. SampleSet.strain_clusters end to end ----
@pytest.fixture(scope="module")
def five_set(ctx):
    """the five samples of test_gpu_compare_set.py (different level sets, one without two scaffolds) under names whose sorted order is
    not their order of insertion; three genomes and a scaffold the stb does not name"""
    from instrain_amd import compare, engine
    from tests.test_gpu_compare_set import LENGTHS, NAMES, SB, Sample
    from tests.test_gpu_parity import _random_split
    seq = re.sub("[^ACGT]", "A", _random_split(700, int(SB[-1]), 5, 1, 10)[0])
    codes = engine.encode_seq(seq)
    samples = [Sample("s2.bam", 701, 30, 1), Sample("s10.bam", 702, 24, 1, drop=(3, 7)), Sample("s1.bam", 703, 26, 4),
               Sample("s0.bam", 704, 28, 3, values=[0, 1, 3]), Sample("s9.bam", 705, 22, 2, values=[0, 2])]
    stb = {"sc0": "gB", "sc1": "gB", "sc2": "gB", "sc3": "gC", "sc4": "gC", "sc7": "gC", "sc5": "gA", "sc8": "gA"}      # sc6: in no genome
    b2l = {}
    for n, ln in zip(NAMES, LENGTHS):
        if n in stb:
            b2l[stb[n]] = b2l.get(stb[n], 0) + ln
    st = compare.SampleSet(ctx, NAMES, LENGTHS, min_cov=5)
    for s in samples:
        b, names, bounds = s.batch(ctx, codes)
        st.add_batch(s.name, b, names, bounds, mm_values=s.values)
        b.close()
    yield dict(st=st, stb=stb, b2l=b2l, names=NAMES, lengths=LENGTHS, samples=[s.name for s in samples])
    st.close()


def test_strain_clusters_end_to_end(ctx, five_set):
    from instrain_amd import _lib, compare
    from instrain_amd._lib import IsxError
    st, stb, b2l = five_set["st"], five_set["stb"], five_set["b2l"]
    with pytest.raises(IsxError) as e:                           # no compare() since the last add_batch
        st.strain_clusters(stb, b2l)
    assert e.value.code == -6
    table = st.compare(min_freq=0.05)
    assert not st.failed
    tol = len(five_set["names"]) * 2.0 ** -52
    mine = cr.genome_pairs(table, stb, five_set["names"])
    dists = np.concatenate([cr.genome_matrix(mine[g], b2l[g], 0.1)[2][np.triu_indices(5, 1)] for g in sorted(mine)])
    assert sorted(mine) == ["gA", "gB", "gC"] and dists.max() > dists.min()
    thresholds = (0.99999, 1.0 - float(np.median(dists)))      # the default, and one that cuts through the middle of the distances
    for method, t in itertools.product(cr.METHODS, thresholds):
        logs = []
        cdb = st.strain_clusters(stb, b2l, ani_threshold=t, coverage_treshold=0.1, clusterAlg=method, logs=logs)
        assert st.cluster_genomes == ["gA", "gB", "gC"] and (st.cluster_status["status"] == _lib.CLUSTER_OK).all() and not logs
        assert st.cluster_status["n_points"].tolist() == [5, 5, 5] and st.cluster_device_ms > 0
        # rule 1: the roll-up against genome_wide on the same rows
        mdb = compare.genome_wide(table, stb, b2l)
        got = st.cluster_pairs()
        pair_at = {p: k for k, p in enumerate(itertools.combinations(five_set["samples"], 2))}
        seen = np.zeros(got.shape, bool)
        for genome, n1, n2, cbc, ani in zip(mdb["genome"], mdb["name1"], mdb["name2"], mdb["compared_bases_count"], mdb["popANI"]):
            r = got[st.cluster_genomes.index(genome), pair_at[(n1, n2)]]
            seen[st.cluster_genomes.index(genome), pair_at[(n1, n2)]] = True
            assert int(r["tcb"]) == int(cbc) and r["n_rows"] > 0 and abs(r["w"] / r["tcb"] - ani) <= tol, (genome, n1, n2)
        assert seen.all() and len(mdb) == got.size
        n_rows = got["n_rows"][st.cluster_genomes.index("gC")]
        assert sorted(set(n_rows.tolist())) == [1, 3]            # the sample without sc3 and sc7 shares one scaffold of gC with the others
        # rules 2-7: the frame form on that table and the restatement on the rows
        exp = cr.strain_clusters(table, stb, five_set["names"], b2l, ani_threshold=t, coverage_treshold=0.1, method=method)
        assert cdb.values.tolist() == [list(r) for r in exp], (method, t)
        frame = compare.cluster_genome_strains(ctx, mdb, ani_threshold=t, coverage_treshold=0.1, clusterAlg=method)
        assert frame.values.tolist() == cdb.values.tolist()
        assert cdb["sample"].tolist()[:5] == sorted(five_set["samples"]) != five_set["samples"]
        for genome in st.cluster_genomes:
            _, names, m = cr.genome_matrix(mine[genome], b2l[genome], 0.1)
            assert st.cluster_linkage(genome).tobytes() == cr.linkage(m[np.triu_indices(5, 1)], 5, method).tobytes(), (genome, method)
    assert len(set(st.strain_clusters(stb, b2l, ani_threshold=0.0)["cluster"])) == 3 < len(set(st.strain_clusters(stb, b2l)["cluster"]))
    # bin2length left out: the summed set lengths of the genome's scaffolds; two calls give the same table
    a, b = st.strain_clusters(stb), st.strain_clusters(stb, b2l)
    assert a.values.tolist() == b.values.tolist()
    # refused on the host, each leaving the set as it was
    with pytest.raises(ValueError):
        st.strain_clusters(stb, b2l, clusterAlg="ward")
    S = len(five_set["samples"])
    sg, ln, rank = np.zeros(len(five_set["names"]), np.int32), np.ones(1), np.arange(S, dtype=np.int32)
    status, labels = np.zeros(1, _lib.CLUSTER_STATUS_DT), np.zeros(S, np.int32)

    def raw(method, sg=sg, rank=rank):
        return st.lib.isx_cmpset_cluster(st.h, 1, sg.ctypes.data, ln.ctypes.data, rank.ctypes.data, method, 1e-5, 0.1, status.ctypes.data,
                                         labels.ctypes.data, None)
    assert raw(b"single") == -1 and raw(b"nearest") == -1 and raw(None) == -1
    assert raw(b"average", sg=sg + 1) == -1 and raw(b"average", rank=rank * 0) == -1       # a genome outside the call; no permutation
    assert raw(b"average") == 0 and status["status"][0] == _lib.CLUSTER_OK
    assert st.strain_clusters(stb, b2l).values.tolist() == b.values.tolist()


def _covered(ctx, lengths, names, ref, cover, depth=12):
    """a run batch of one sample: `depth` reads showing the reference on every position of cover[scaffold] = (first, end)"""
    from instrain_amd import engine
    from tests.test_gpu_compare_set import _batch
    sb = np.r_[0, np.cumsum(lengths)]
    pos = np.concatenate([np.repeat(np.arange(sb[k] + a, sb[k] + b), depth) for k, (a, b) in enumerate(cover)] + [np.zeros(0, np.int64)])
    return _batch(ctx, engine.encode_seq("".join("ACTG"[c] for c in ref)), sb, pos, ref[pos], np.zeros(len(pos), np.int64), 1)


def test_genomes_that_are_not_clustered(ctx):
    """rule 3a (a pair that compared no base) and rule 3b (two samples that share no scaffold of the genome): that genome alone is
    skipped, with its line, and the others keep consecutive numbers"""
    from instrain_amd import _lib, compare
    names, lengths = ["ok1", "p", "q", "z", "ok2"], [150, 100, 100, 200, 90]
    stb = {"ok1": "g1_fine", "p": "g2_missing", "q": "g2_missing", "z": "g3_zero", "ok2": "g4_fine"}
    ref = np.random.Generator(np.random.PCG64(9)).integers(0, 4, size=sum(lengths)).astype(np.uint8)
    full = [(0, n) for n in lengths]
    cover = {"A": [full[0], full[1], (0, 0), (0, 100), full[4]],         # A and B meet on no scaffold of g2, and on no base of z
             "B": [full[0], (0, 0), full[2], (100, 200), full[4]],
             "C": full}
    st = compare.SampleSet(ctx, names, lengths, min_cov=5)
    for s in "ABC":
        b = _covered(ctx, lengths, names, ref, cover[s])
        st.add_batch(s, b, names, np.r_[0, np.cumsum(lengths)])
        b.close()
    table = st.compare()
    assert any(r["scaffold"] == "z" and r["compared_bases_count"] == 0 for r in table)
    logs = []
    cdb = st.strain_clusters(stb, logs=logs)
    assert st.cluster_status["status"].tolist() == [_lib.CLUSTER_OK, _lib.CLUSTER_MISSING_PAIR, _lib.CLUSTER_NO_OVERLAP, _lib.CLUSTER_OK]
    assert cdb.values.tolist() == [["1_1", s, "g1_fine"] for s in "ABC"] + [["2_1", s, "g4_fine"] for s in "ABC"]
    assert len(logs) == 2 and "g2_missing" in logs[0] and "never compared" in logs[0] and logs[1].startswith("Cannot cluster genome g3_zero")
    pairs = st.cluster_pairs()                                   # pairs (A,B), (A,C), (B,C)
    assert pairs["n_rows"].tolist() == [[1, 1, 1], [0, 1, 1], [1, 1, 1], [1, 1, 1]]
    assert pairs["tcb"].tolist() == [[150] * 3, [0, 100, 100], [0, 100, 100], [90] * 3]
    exp_logs = []
    exp = cr.strain_clusters(table, stb, names, {"g1_fine": 150, "g2_missing": 200, "g3_zero": 200, "g4_fine": 90}, logs=exp_logs)
    assert [list(r) for r in exp] == cdb.values.tolist() and exp_logs == logs
    with pytest.raises(_lib.IsxError):                           # a genome that was not clustered has no linkage to fetch
        st.cluster_linkage("g3_zero")
    st.close()


def test_a_failed_scaffold_is_left_out(ctx):
    """the scaffold on which a pair fails (an N reference base under a lone SNV row) gives no row to any pair: its bases are not in tcb"""
    from instrain_amd import compare, engine
    from tests.test_gpu_compare_set import _batch
    lengths, depth = [300, 200], 12
    sb = np.r_[0, np.cumsum(lengths)]
    ref = np.random.Generator(np.random.PCG64(55)).integers(0, 4, size=int(sb[-1])).astype(np.uint8)
    seq = "".join("ACTG"[c] for c in ref)
    codes = engine.encode_seq(seq[:100] + "N" + seq[101:])
    st = compare.SampleSet(ctx, ["n", "ok"], lengths, min_cov=5)
    for name, n_at in (("A", True), ("B", False), ("C", True)):
        pos = np.repeat(np.arange(int(sb[-1])), depth)
        base = ref[pos].copy()
        base[pos == 100] = 0
        keep = np.ones(len(pos), bool) if n_at else pos != 100
        b = _batch(ctx, codes, sb, pos[keep], base[keep], np.zeros(int(keep.sum()), np.int64), 1)
        st.add_batch(name, b, ["n", "ok"], sb)
        b.close()
    table = st.compare()
    assert st.failed == {0} and {r["scaffold"] for r in table} == {"ok"}
    cdb = st.strain_clusters({"n": "g", "ok": "g"})
    pairs = st.cluster_pairs()
    assert pairs["tcb"].tolist() == [[200, 200, 200]] and pairs["n_rows"].tolist() == [[1, 1, 1]]
    assert cdb.values.tolist() == [["1_1", s, "g"] for s in "ABC"]
    st.close()


# ---- 4. refused arguments ----
def test_refused_arguments(ctx):
    from instrain_amd import _lib, compare
    from instrain_amd._lib import IsxError
    good = np.array([0.0, 0.5, 0.25])
    with pytest.raises(ValueError):
        compare.linkage_flat(ctx, [good], "centroid", 0.1)
    with pytest.raises(ValueError):                              # four values are no condensed matrix; a square one must be symmetric
        compare.linkage_flat(ctx, [np.zeros(4)], "average", 0.1)
    with pytest.raises(ValueError):
        compare.linkage_flat(ctx, [np.array([[0.0, 1.0], [2.0, 0.0]])], "average", 0.1)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(IsxError) as e:
            compare.linkage_flat(ctx, [good, np.array([0.1, bad, 0.3])], "average", 0.1)
        assert e.value.code == -1 and "problem 1" in str(e.value)
    big = _lib.CLUSTER_MAX_POINTS + 1
    with pytest.raises(IsxError) as e:
        compare.linkage_flat(ctx, [np.zeros(big * (big - 1) // 2)], "average", 0.1)
    assert e.value.code == _lib.ERR_CAPACITY

    def raw(method, n_points, offsets, values):
        n_points, offsets = np.array(n_points, np.int32), np.array(offsets, np.int64)
        labels = np.zeros(int(n_points.sum()), np.int32)
        return ctx.lib.isx_cluster_linkage(ctx.h, len(n_points), n_points.ctypes.data, offsets.ctypes.data, values.ctypes.data, len(values),
                                           method, 0.1, labels.ctypes.data, None, C.byref(C.c_float(0)))
    for name in cr.REFUSED + ("nearest",):
        assert raw(name.encode(), [3], [0], good) == -1
    assert "not supported" in ctx.lib.isx_last_error().decode()
    assert raw(b"average", [4], [0], good) == -1                 # six values needed, three given
    assert raw(b"average", [3], [1], good) == -1                 # the matrix would end behind the values
    assert raw(b"average", [3], [-1], good) == -1
    assert raw(b"average", [1], [0], good) == -1                 # fewer than two points
    assert raw(b"average", [3], [0], good) == 0
    (lab, Z), = compare.linkage_flat(ctx, [good], "average", 0.3)                          # the context is as usable as before
    elab, eZ = cr.linkage_flat(good, "average", 0.3)
    assert lab.tolist() == elab.tolist() == [1, 1, 2] and Z.tobytes() == eZ.tobytes()
