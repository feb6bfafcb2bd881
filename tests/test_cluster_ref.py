"""CPU-only: tests/cluster_ref.py, the numpy restatement of strain clustering, against the reference's own vectors
(tests/golden/make_cluster_golden.py: Mdb, Cdb, per genome the matrix with scipy's Z and labels) and against scipy itself on matrices
full of ties.  The device path (tests/test_gpu_cluster.py) is then held to this restatement bit for bit."""
import json
import os

import numpy as np
import pandas as pd
import pytest

from tests import cluster_ref as cr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden():
    g = json.load(open(os.path.join(GOLDEN, "cluster_golden.json")))
    g["table"] = pd.read_csv(os.path.join(GOLDEN, "cluster_table.csv"), float_precision="round_trip")
    g["mdb"] = pd.read_csv(os.path.join(GOLDEN, "cluster_mdb.csv"), float_precision="round_trip")
    g["order"] = [n for n, _ in g["scaffolds"]]
    # ten times what the generator saw between the reference and the restatement, at least the reordering error of rule 1's sum
    g["tol"] = max(10.0 * g["max_abs_diff"], len(g["scaffolds"]) * 2.0 ** -52)
    return g


@pytest.fixture(scope="module")
def golden():
    return load_golden()


def cases(g):
    return [(m, t) for m in cr.METHODS for t in g["thresholds"]]


def test_fixture_holds_what_it_is_for(golden):
    g = golden
    assert sorted(g["samples"]) != g["samples"] and len(g["samples"]) == 9
    assert "gD_zero" not in g["genomes"] and (g["mdb"][g["mdb"]["genome"] == "gD_zero"]["compared_bases_count"] == 0).any()
    assert sorted(set(g["mdb"]["genome"])).index("gD_zero") not in (0, len(set(g["mdb"]["genome"])) - 1)
    assert all(v == 0 for v in g["genomes"]["gA_same"]["condensed"]) and len(g["genomes"]["gA_same"]["samples"]) == 9
    assert 1.0 in g["genomes"]["gB_two"]["condensed"] and len(g["genomes"]["gE_pair"]["samples"]) == 2
    assert sorted(g["genomes"]["gC_chain"]["condensed"])[:2] == [0, 0] and max(g["genomes"]["gC_chain"]["condensed"]) > 1e-5
    assert set(g["table"]["scaffold"]) - set(g["stb"]) == {"free_1"}
    assert g["table"][g["table"]["scaffold"].map(g["stb"]) == "gF_subset"]["popANI"].isna().any()
    assert g["max_abs_diff"] <= 1e-12
    # the thresholds decide something: the two cutoffs give different tables
    assert g["cdb"]["average 0.99999"] != g["cdb"]["average 0.999"]


def test_linkage_and_labels_equal_scipys_exactly_given_the_matrix(golden):
    for genome, e in golden["genomes"].items():
        n = len(e["samples"])
        for method in cr.METHODS:
            Z = cr.linkage(e["condensed"], n, method)
            assert Z.tobytes() == np.array(e["Z"][method], dtype=np.float64).tobytes(), (genome, method)
            for t in golden["thresholds"]:
                assert cr.fcluster(Z, n, 1.0 - t).tolist() == e["labels"][method]["%r" % t], (genome, method, t)


def test_rules_1_to_4_give_the_references_matrices(golden):
    g = golden
    pairs = cr.genome_pairs(g["table"].to_dict("records"), g["stb"], g["order"])
    assert sorted(pairs) == sorted(set(g["mdb"]["genome"]))
    for genome, p in pairs.items():
        status, samples, m = cr.genome_matrix(p, g["bin2length"][genome], g["coverage_treshold"])
        rows = g["mdb"][g["mdb"]["genome"] == genome]
        assert {k: v[0] for k, v in p.items()} == {(a, b): c for a, b, c in zip(rows["name1"], rows["name2"], rows["compared_bases_count"])}
        if genome == "gD_zero":
            assert status == cr.NO_OVERLAP
            continue
        assert status == cr.OK and samples == g["genomes"][genome]["samples"] == sorted(samples)
        np.testing.assert_allclose(m[np.triu_indices(len(samples), 1)], g["genomes"][genome]["condensed"], rtol=0, atol=g["tol"])
    # ... and the frame form (a stored genomeWide_compare table) the same ones
    for genome, (status, samples, m) in cr.frame_matrices(g["mdb"], g["coverage_treshold"]).items():
        if genome == "gD_zero":
            assert status == cr.NO_OVERLAP
        else:
            assert m[np.triu_indices(len(samples), 1)].tolist() == g["genomes"][genome]["condensed"]


def test_the_table_equals_the_references(golden):
    g = golden
    for method, t in cases(g):
        logs = []
        rows = cr.strain_clusters(g["table"].to_dict("records"), g["stb"], g["order"], g["bin2length"], ani_threshold=t,
                                  coverage_treshold=g["coverage_treshold"], method=method, logs=logs)
        assert [list(r) for r in rows] == g["cdb"]["%s %r" % (method, t)], (method, t)
        assert len(logs) == 1 and logs[0].startswith("Cannot cluster genome gD_zero")
        frame = cr.cluster_rows(cr.frame_matrices(g["mdb"], g["coverage_treshold"]), method, 1.0 - t)
        assert [list(r) for r in frame] == g["cdb"]["%s %r" % (method, t)]


def test_a_missing_pair_skips_that_genome_alone(golden):
    g = golden
    mdb = g["mdb"]
    cut = mdb[~((mdb["genome"] == "gB_two") & (mdb["name1"] == "s2.bam") & (mdb["name2"] == "s3.bam"))]
    mats = cr.frame_matrices(cut, g["coverage_treshold"])
    assert mats["gB_two"][0] == cr.MISSING_PAIR
    logs = []
    rows = cr.cluster_rows(mats, "average", 1e-5, logs)
    assert [r[2] for r in rows].count("gB_two") == 0 and len(logs) == 2 and any("gB_two" in ln and "never compared" in ln for ln in logs)
    assert sorted({r[0].split("_")[0] for r in rows}) == ["1", "2", "3", "4"]                  # the others keep consecutive numbers
    assert {r[2]: r[0].split("_")[0] for r in rows} == {"gA_same": "1", "gC_chain": "2", "gE_pair": "3", "gF_subset": "4"}


def tie_heavy_matrices(seed, sizes, per_size=3):
    """seeded condensed matrices of the kinds that are full of ties: few distinct values, uniform, zeros and ones only"""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for n in sizes:
        m = n * (n - 1) // 2
        for kind in range(per_size):
            if kind % 3 == 0:
                v = rng.choice([0.0, 1e-6, 2e-5, 3e-4, 1.0], size=m)
            elif kind % 3 == 1:
                v = rng.random(m)
            else:
                v = rng.choice([0.0, 1.0], size=m)
            out.append((n, v))
    return out


def test_restatement_equals_scipy_on_tie_heavy_matrices():
    sch = pytest.importorskip("scipy.cluster.hierarchy")
    n_done = 0
    for n, v in tie_heavy_matrices(77, list(range(2, 14)) * 4 + [31, 40]):
        for method in cr.METHODS:
            Z, ref = cr.linkage(v, n, method), sch.linkage(v, method=method)
            assert Z.tobytes() == ref.tobytes(), (n, method)
            for cutoff in (1.0 - 0.99999, 2e-5, 0.5):
                assert cr.fcluster(Z, n, cutoff).tolist() == sch.fcluster(ref, cutoff, criterion="distance").tolist(), (n, method, cutoff)
            n_done += 1
    assert n_done > 400


def test_refused_methods():
    from instrain_amd import compare
    for name in cr.REFUSED + ("nearest", ""):
        with pytest.raises(ValueError):
            cr.linkage([0.5], 2, name)
        with pytest.raises(ValueError):                                                       # refused before anything touches a device
            compare.linkage_flat(None, [np.zeros((2, 2))], name, 0.1)
        with pytest.raises(ValueError):
            compare.cluster_genome_strains(None, pd.DataFrame(), clusterAlg=name)
    assert compare._lib.CLUSTER_METHODS == cr.METHODS and compare._lib.CLUSTER_LDS_MAX_POINTS >= 128
