"""Inputs of tests/test_gpu_bs16_planes.py and tests/run_bs16_planes_tree.py: the clique tree and the Bethe graph of a 4-tip or
5-tip caterpillar tree with random symmetric positive-definite cluster beliefs (every entry different from every other, so
that a block, a column or a plane read from the wrong place shows)."""
import numpy as np

from pgbp_amd import synth as S


def caterpillar(ntips):
    """(((t, t), t), ...) in preorder: spine 0 .. ntips-2, the cherry of the last spine node, then one tip per spine node on
    the way back up.  4 tips: the 2p-dimensional cluster {2, 1} receives a cherry; 5 tips: {2, 1} receives one leaf message
    and the message of the internal cluster {3, 2}; the tip below the root makes a cluster of dimension 0 (a constant)."""
    n = ntips
    N = 2 * n - 1
    parent = np.full(N, -1, dtype=np.int64)
    for i in range(1, n - 1):
        parent[i] = i - 1
    parent[n - 1] = parent[n] = n - 2
    for j in range(1, n - 1):
        parent[n + j] = n - 2 - j
    is_leaf = np.ones(N, dtype=bool)
    is_leaf[parent[1:]] = False
    length = np.linspace(0.3, 0.9, N)
    length[0] = 0.0
    return S.Tree(parent, length, is_leaf)


def spd_packed(prob, rng):
    """packed (J, h, g) records: every cluster a random symmetric (exactly) positive-definite J, random h and g; sepsets 0"""
    out = np.zeros(int(prob.packed_off[-1]))
    for i in range(prob.nclusters):
        m, o = int(prob.dims[i]), int(prob.packed_off[i])
        A = rng.standard_normal((m, m))
        J = A @ A.T + m * np.eye(m)
        J = (J + J.T) / 2
        out[o:o + m * m] = J.reshape(-1, order="F")
        out[o + m * m:o + m * m + m] = rng.standard_normal(m)
        out[o + m * m + m] = rng.standard_normal()
    assert len(np.unique(out[out != 0.0])) >= np.count_nonzero(out) - sum(
        int(m) * (int(m) - 1) // 2 for m in prob.dims[:prob.nclusters]), "entries are not all distinct"
    return out


def cliquetree_case(ntips, p, n_sites, seed=0):
    tr = caterpillar(ntips)
    prob = S.cliquetree_of_tree(tr, p)
    rng = np.random.default_rng(1000 * p + 10 * ntips + seed)
    return prob, [spd_packed(prob, rng) for _ in range(n_sites)]


def bethe_case(ntips, p, seed=0):
    tr = caterpillar(ntips)
    prob = S.bethe_of_tree(tr, p)
    rng = np.random.default_rng(7000 + 1000 * p + 10 * ntips + seed)
    return prob, [spd_packed(prob, rng)]
