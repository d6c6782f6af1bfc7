"""CPU oracle of Gallery.dbscan (dif_gallery_dbscan), on cluster_ref.lower_distances.  TEST INFRASTRUCTURE ONLY.

    E = {(i, j) : j < i and distance(rows[i][None, :], rows[j][None, :], metric) <= t}
          # i is the probe, reference float32 values, inclusive, NaN <= t is False; `clamp` as in cluster_ref; no self pairs
    degree[i] = 1 + number of edges of E that contain i          # the row itself always counts
    core[i]   = degree[i] >= min_samples
    clusters  = connected components of the graph (core rows, edges of E with both ends core)
    label[c]  = index_base + smallest row of c's component       for a core row c
    label[b]  = label[a(b)]                                      for a non-core row b with at least one core neighbour:
          # a(b) = the core neighbour with the smallest float32 distance (the edge's value), exact ties to the lower row
    label[x]  = -1 for every other row (noise), whatever index_base is
    counts    = (number of clusters, number of noise rows)

Also the rows the dbscan tests run on (`make_rows`): identities of 1-6 rows built so that core, border and noise rows all occur."""
import math

import numpy as np

import cluster_ref as cr


def edges_from(lower, t):
    """-> (i [E], j [E], d [E] float32): the edges j < i of `lower` (cluster_ref.lower_distances) at tolerance t, by probe."""
    t = np.float32(t)
    ii, jj, dd = [], [], []
    with np.errstate(invalid='ignore'):
        for i, d in enumerate(lower):
            js = np.flatnonzero(d[:i] <= t)                       # d[i] is the self pair: not an edge
            ii.append(np.full(js.size, i, dtype=np.int64))
            jj.append(js.astype(np.int64))
            dd.append(np.asarray(d[js], dtype=np.float32))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dtype=dt)
    return cat(ii, np.int64), cat(jj, np.int64), cat(dd, np.float32)


def dbscan_from(lower, G, t, min_samples, index_base=0):
    """-> (labels [G] int64, degree [G] int32, counts (clusters, noise)) from cluster_ref.lower_distances' list."""
    ei, ej, ed = edges_from(lower, t)
    degree = np.ones(G, dtype=np.int64)
    np.add.at(degree, ei, 1)
    np.add.at(degree, ej, 1)
    core = degree >= min_samples
    parent = np.arange(G, dtype=np.int64)

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    both = core[ei] & core[ej]
    for i, j in zip(ei[both], ej[both]):
        a, b = find(int(i)), find(int(j))
        if a != b:
            parent[max(a, b)] = min(a, b)                         # (any rule would do: the labels below are canonical)
    root = np.array([find(i) for i in range(G)], dtype=np.int64)
    low = np.full(G, G, dtype=np.int64)
    np.minimum.at(low, root[core], np.flatnonzero(core))         # the smallest row of every core component
    labels = np.full(G, -1, dtype=np.int64)
    labels[core] = index_base + low[root[core]]
    # border rows: the nearest core neighbour by (float32 bits of the distance, row).  Both metrics only give distances >= +0
    # (a sum of squares; arccos(.) / pi), so the bit pattern orders like the value: asserted on every distance compared.
    best = {}
    for i, j, d in zip(ei, ej, ed):
        for b, c in ((int(i), int(j)), (int(j), int(i))):
            if core[b] or not core[c]:
                continue
            bits = int(np.float32(d).view(np.uint32))
            assert d >= 0 and bits < 0x80000000, (i, j, d)        # not -0, not negative: bits order like the value
            key = (bits, c)
            if b not in best or key < best[b]:
                best[b] = key
    for b, (_, c) in best.items():
        labels[b] = labels[c]
    n_clusters = int(len(np.unique(root[core])))
    return labels, degree.astype(np.int32), (n_clusters, int((labels == -1).sum()))


def dbscan(rows, t, min_samples, metric, clamp=False, index_base=0):
    rows = np.asarray(rows, dtype=np.float32)
    return dbscan_from(cr.lower_distances(rows, metric, clamp), rows.shape[0], t, min_samples, index_base)


def kinds(labels, degree, min_samples):
    """-> (core, border, noise) Boolean masks of a result."""
    core = np.asarray(degree) >= min_samples
    noise = np.asarray(labels) == -1
    return core, ~core & ~noise, noise


# ------------------------------------------------------------------------------------------------ the rows of the tests
# Distances are placed, not drawn.  Around a unit centre c with orthonormal directions e_k (all orthogonal to c):
#   c + r e_k            lies at distance `v` from c           for r = _r_centre(v)
#   c + r e_a, c + r e_b lie at distance `v` from each other   for r = _r_pair(v)   (and between v_a and v_b for two radii)
# in the units of the metric (0: squared L2; 1: arccos(similarity) / pi).  Edge distances are drawn from EDGE[metric]; the
# nearest non-edges inside an identity (two leaves of a star) fall into NEAR[metric], above EDGE by the widest gap there is:
# a ladder of single rows around the first centre, LADDER[metric] apart, fills the range up to the strangers' distances.
EDGE = {0: (0.162, 0.2), 1: (0.1226, 0.1348)}
NEAR = {0: (0.324, 0.4), 1: (0.1711, 0.1873)}
LADDER = {0: (0.1, 2.0), 1: (0.03, 0.5)}                          # step, end


def _r_centre(v, metric):
    return math.sqrt(v) if metric == 0 else math.tan(math.pi * v)


def _r_pair(v, metric):
    return math.sqrt(v / 2) if metric == 0 else math.sqrt(1 / math.cos(math.pi * v) - 1)


def make_rows(G, D, metric, seed=0):
    """G rows of identities with 1-6 rows each, in a shuffled order (an identity's rows lie anywhere in the gallery):
      star k    a centre and k = 3, 4, 5 leaves, each an edge away from the centre and a non-edge from each other: at
                min_samples = 4 the centre is core and the leaves are border rows;
      clique s  s = 1 .. 6 rows, every pair an edge: all core or (s < min_samples) all noise;
    and, from 127 rows up, the ladder of single rows (noise) that makes the gap above the edges the widest one."""
    rng = np.random.default_rng(100000 * seed + 1000 * G + 10 * D + metric)
    lo, hi = EDGE[metric]
    out = []
    plan = [('star', 3), ('clique', 1), ('clique', 5), ('star', 5), ('clique', 2), ('clique', 4), ('clique', 3), ('star', 4),
            ('clique', 6)]
    first = True
    k = 0
    while len(out) < G:
        kind, n = plan[k % len(plan)]
        k += 1
        ladder = []
        if first and G >= 127:
            step, end = LADDER[metric]
            ladder = list(np.arange(NEAR[metric][1] + step, end, step))
        basis = np.linalg.qr(rng.standard_normal((D, 1 + 6 + len(ladder))))[0].T   # orthonormal rows: c, e_0 .. e_5, ladder
        c = basis[0]
        if kind == 'star':
            out.append(c)
            out += [c + _r_centre(rng.uniform(lo, hi), metric) * basis[1 + a] for a in range(n)]
        else:
            out += [c + _r_pair(rng.uniform(lo, hi), metric) * basis[1 + a] for a in range(n)]
        out += [c + _r_centre(v, metric) * basis[7 + a] for a, v in enumerate(ladder)]
        first = False
    rows = np.asarray(out[:G], dtype=np.float64)
    rows = rows[rng.permutation(G)].astype(np.float32)
    rows.setflags(write=False)
    return rows


def bridge_rows(bridge_x, swap, k=3, D=32, seed=4):
    """The chaining case, metric 0, exact float32 coordinates, t = 1, min_samples = 4: a core cA at (-1, 0, ...) with k
    companions at (-1.5, 0, ...), cB and its companions mirrored at +1 / +1.5, a bridge row at (bridge_x, 0, ...) and one far
    row, stored in a shuffled order; `swap` exchanges the places of cA and cB.  -> (rows, {name: row number(s)})."""
    n = 2 * (k + 1) + 2
    perm = np.random.default_rng(seed).permutation(n)
    names = {'cA': perm[0], 'A': perm[1:1 + k], 'cB': perm[1 + k], 'B': perm[2 + k:2 + 2 * k], 'bridge': perm[n - 2], 'far': perm[n - 1]}
    if swap:
        names['cA'], names['cB'] = names['cB'], names['cA']
    rows = np.zeros((n, D), dtype=np.float32)
    rows[names['cA'], 0], rows[names['A'], 0] = -1.0, -1.5
    rows[names['cB'], 0], rows[names['B'], 0] = 1.0, 1.5
    rows[names['bridge'], 0] = bridge_x
    rows[names['far'], 1] = 100.0
    return rows, names
