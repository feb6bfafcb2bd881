"""Plain numpy / Python restatement of strain clustering (`inStrain compare`'s strain_clusters.tsv), the yardstick of the device path
(instrain_amd/csrc/isx_cluster.hip).  Test infrastructure: nothing here is imported by the package.

    rule 1    genome roll-up of a pair            genomeUtilities.py:739-800 with mm_level off
    rule 2-4  samples, skipped genomes, distance  compare_utils.py:169-268
    rule 5    scipy.cluster.hierarchy.linkage for average / complete / weighted: the NN-chain, its stable sort and its relabel
    rule 6    scipy.cluster.hierarchy.fcluster(criterion='distance')
    rule 7    the Cdb table                       compare_utils.py:205-255

Every float is an IEEE double made by one operation at a time in a fixed order, so a device that does the same gives the same bits."""
import itertools

import numpy as np

METHODS = ("average", "complete", "weighted")
REFUSED = ("single", "centroid", "median", "ward")      # scipy runs other algorithms for these
OK, NO_OVERLAP, MISSING_PAIR = 0, 1, 2                  # a genome: clustered, rule 3a, rule 3b


def check_method(method):
    if method not in METHODS:
        raise ValueError("clustering method %r is not supported (supported: %s)" % (method, ", ".join(METHODS)))
    return METHODS.index(method)


def condensed_index(n, i, j):
    if i > j:
        i, j = j, i
    return n * i - i * (i + 1) // 2 + (j - i - 1)


def _new_dist(method, d_xi, d_yi, nx, ny):
    if method == "average":
        return (np.float64(nx) * d_xi + np.float64(ny) * d_yi) / np.float64(nx + ny)
    if method == "complete":
        return d_xi if d_xi > d_yi else d_yi
    return (d_xi + d_yi) / np.float64(2.0)


def linkage(condensed, n, method):
    """-> Z[n - 1, 4] as scipy.cluster.hierarchy.linkage(condensed, method) (rule 5)"""
    check_method(method)
    D = np.array(condensed, dtype=np.float64)
    assert n >= 2 and len(D) == n * (n - 1) // 2
    size = [1] * n
    chain, raw = [], []
    for _ in range(n - 1):
        if not chain:
            chain.append(next(i for i in range(n) if size[i] > 0))
        for _scan in range(2 * n + 1):
            x = chain[-1]
            if len(chain) > 1:
                y = chain[-2]
                cur = D[condensed_index(n, x, y)]
            else:
                y, cur = -1, np.float64(np.inf)
            for i in range(n):
                if size[i] == 0 or i == x:
                    continue
                d = D[condensed_index(n, x, i)]
                if d < cur:
                    cur, y = d, i
            if len(chain) > 1 and y == chain[-2]:
                break
            chain.append(y)
        else:
            raise RuntimeError("the chain did not close")
        del chain[-2:]
        if x > y:
            x, y = y, x
        nx, ny = size[x], size[y]
        raw.append((x, y, cur, nx + ny))
        size[x], size[y] = 0, nx + ny
        for i in range(n):
            if size[i] == 0 or i == y:
                continue
            D[condensed_index(n, i, y)] = _new_dist(method, D[condensed_index(n, i, x)], D[condensed_index(n, i, y)], nx, ny)
    order = sorted(range(n - 1), key=lambda k: raw[k][2])           # (stable)
    Z = np.zeros((n - 1, 4), dtype=np.float64)
    parent = list(range(2 * n - 1))
    count = [1] * (2 * n - 1)

    def find(v):
        while parent[v] != v:
            v = parent[v]
        return v

    for k, o in enumerate(order):
        a, b = find(raw[o][0]), find(raw[o][1])
        if a > b:
            a, b = b, a
        parent[a] = parent[b] = n + k
        count[n + k] = count[a] + count[b]
        Z[k] = (a, b, raw[o][2], count[n + k])
    return Z


def fcluster(Z, n, cutoff):
    """-> labels[n] as scipy.cluster.hierarchy.fcluster(Z, cutoff, criterion='distance') (rule 6)"""
    left, right = Z[:, 0].astype(np.int64), Z[:, 1].astype(np.int64)
    crit = np.zeros(n - 1, dtype=np.float64)
    for k in range(n - 1):
        m = Z[k, 2]
        for c in (left[k], right[k]):
            if c >= n and crit[c - n] > m:
                m = crit[c - n]
        crit[k] = m
    labels = np.zeros(n, dtype=np.int32)
    visited = [False] * (n - 1)
    stack, leader, n_cluster = [n - 2], -1, 0
    while stack:
        root = stack[-1]
        lc, rc = int(left[root]), int(right[root])
        if leader == -1 and crit[root] <= cutoff:
            leader, n_cluster = root, n_cluster + 1
        if lc >= n and not visited[lc - n]:
            visited[lc - n] = True
            stack.append(lc - n)
            continue
        if rc >= n and not visited[rc - n]:
            visited[rc - n] = True
            stack.append(rc - n)
            continue
        for c in (lc, rc):
            if c < n:
                if leader == -1:
                    n_cluster += 1
                labels[c] = n_cluster
        if leader == root:
            leader = -1
        stack.pop()
    return labels


def linkage_flat(matrix, method, cutoff):
    """square or condensed distances -> (labels, Z)"""
    m = np.asarray(matrix, dtype=np.float64)
    if m.ndim == 2:
        n = len(m)
        m = m[np.triu_indices(n, 1)]
    else:
        n = int(round((1 + np.sqrt(1 + 8 * len(m))) / 2))
    Z = linkage(m, n, method)
    return fcluster(Z, n, cutoff), Z


# ---- rules 1-4: from scaffold rows to a genome's matrix ----
def last_rows(table):
    """the highest-mm row of every (scaffold, name1, name2) (the reference's "sort by mm, keep last"), in order of first appearance"""
    best = {}
    for r in table:
        k = (r["scaffold"], r["name1"], r["name2"])
        if k not in best or r["mm"] >= best[k]["mm"]:
            best[k] = r
    return best


def genome_pairs(table, stb, scaffold_order):
    """rule 1 -> {genome: {(name1, name2): (tcb, w, n_rows)}}; the rows of a (genome, pair) are summed in `scaffold_order`"""
    best = last_rows(table)
    place = {s: i for i, s in enumerate(scaffold_order)}
    out = {}
    for (scaffold, n1, n2), r in sorted(best.items(), key=lambda kv: place[kv[0][0]]):
        if scaffold not in stb:
            continue
        tcb, w, k = out.setdefault(stb[scaffold], {}).get((n1, n2), (0, np.float64(0.0), 0))
        both, pop = int(r["compared_bases_count"]), int(r["population_SNPs"])
        if both > 0:
            w = w + (np.float64(both - pop) / np.float64(both)) * np.float64(both)
        out[stb[scaffold]][(n1, n2)] = (tcb + both, w, k + 1)
    return out


def genome_matrix(pairs, length, coverage_treshold):
    """rules 2-4 for one genome: {(name1, name2): (tcb, w, n_rows)} -> (status, samples sorted, square matrix or None)"""
    samples = sorted({n for p in pairs for n in p})
    if any(v[0] == 0 for v in pairs.values()):
        return NO_OVERLAP, samples, None
    n = len(samples)
    m = np.zeros((n, n), dtype=np.float64)
    for a, b in itertools.combinations(range(n), 2):
        v = pairs.get((samples[a], samples[b]), pairs.get((samples[b], samples[a])))
        if v is None:
            return MISSING_PAIR, samples, None
        with np.errstate(divide="ignore", invalid="ignore"):
            pc = np.float64(v[0]) / np.float64(length)
        d = np.float64(1.0) if pc < coverage_treshold else np.float64(1.0) - v[1] / np.float64(v[0])
        m[a, b] = m[b, a] = d
    return OK, samples, m


def cluster_rows(genomes, method, cutoff, logs=None):
    """rule 7.  genomes: {genome: (status, samples, matrix)} -> [(cluster, sample, genome)]"""
    rows, k = [], 0
    for g in sorted(genomes):
        status, samples, m = genomes[g]
        if status != OK:
            if logs is not None:
                logs.append(skip_line(g, status))
            continue
        k += 1
        labels, _ = linkage_flat(m, method, cutoff)
        rows += [("%d_%d" % (k, lab), s, g) for lab, s in zip(labels.tolist(), samples)]
    return rows


def skip_line(genome, status):
    if status == NO_OVERLAP:
        return "Cannot cluster genome %s; some comparisons involve no genomic overlap at all" % (genome,)
    return "Cannot cluster genome %s; some pair of its samples was never compared (not every pair shares a scaffold of it)" % (genome,)


def strain_clusters(table, stb, scaffold_order, bin2length, ani_threshold=0.99999, coverage_treshold=0.1, method="average", logs=None):
    """rules 1-7 from comparisonsTable rows (dicts)"""
    check_method(method)
    gp = genome_pairs(table, stb, scaffold_order)
    genomes = {g: genome_matrix(p, bin2length.get(g, np.nan), coverage_treshold) for g, p in gp.items()}
    return cluster_rows(genomes, method, 1.0 - ani_threshold, logs)


def frame_matrices(Mdb, coverage_treshold):
    """a genome_wide / genomeWide_compare frame -> {genome: (status, samples, matrix)} (rules 2-4 from stored popANI / percent_compared)"""
    out = {}
    for g, gdb in Mdb.groupby("genome"):
        samples = sorted(set(gdb["name1"]) | set(gdb["name2"]))
        if (gdb["compared_bases_count"] == 0).any():
            out[g] = (NO_OVERLAP, samples, None)
            continue
        n, at = len(samples), {s: i for i, s in enumerate(samples)}
        m = np.full((n, n), np.nan)
        np.fill_diagonal(m, 0.0)
        for n1, n2, ani, pc in zip(gdb["name1"], gdb["name2"], gdb["popANI"].astype(np.float64), gdb["percent_compared"].astype(np.float64)):
            d = np.float64(1.0) if pc < coverage_treshold else np.float64(1.0) - ani
            m[at[n1], at[n2]] = m[at[n2], at[n1]] = d
        out[g] = (MISSING_PAIR, samples, None) if np.isnan(m).any() else (OK, samples, m)
    return out
