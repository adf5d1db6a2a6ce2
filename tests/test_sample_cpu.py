"""The preorder conditional sweep of pgbp_sample_posterior, host side (no GPU): tests/sample_ref.py, the plain numpy
restatement of the header's semantics, against the DENSE oracle (oracle/densemvn.py: posterior_node_moments -- the joint
posterior mean and covariance of every node, no message passing).

Inputs: the golden 4-tip tree with 2 traits (missing values, a dimension-0 sepset) and the golden level-1 network's clique
tree, each with its fixed root and with a random root, calibrated by the numpy oracle.  With z = 0 every in-scope variable
is the oracle's posterior mean; with z = [0; I_D] (D = the sample size) A = X[1:] - X[0] holds the square root of the law and
A'A is the oracle's posterior covariance on every pair of in-scope variables, across clusters as well -- which only a
correct JOINT sampler passes, whatever its Cholesky convention.  Bound: 1e-8 relative to the largest entry (the project's
parity bound).  Measured: mean <= 3.9e-16, covariance <= 8.5e-16 over the four cases."""
import numpy as np
import pytest

from helpers import goldens, make_model, oracle_setup
from oracle import beliefs as OB
from oracle import calibration as OC
from oracle import clustergraph as OCG
from oracle import densemvn as OD
from oracle import network as ON
from sample_ref import arrays_from_beliefs, law_errors, sample_posterior_ref, sample_size, unit_draws, variable_nodes

G = goldens()

CASES = {
    "tree_2traits_fixed_root": ("calibration_tree_2traits_missing", ["y1", "y2"], None),
    "tree_2traits_random_root": ("calibration_tree_2traits_missing", ["y1", "y2"], [0.7, 1.3]),
    "level1_network_fixed_root": ("canonicalform_six_messages", ["y"], None),
    "level1_network_random_root": ("canonicalform_six_messages", ["y"], 0.8),
}


def calibrated_case(name):
    """(net, model, tbl, taxa, calibrated oracle ClusterGraphBelief, spanning tree) of one case"""
    key, traits, v = CASES[name]
    g = G[key]
    md = dict(g["model"])
    if v is not None:
        md["v"] = v
    model = make_model(md)
    net = ON.read_newick(g["net"])
    tbl = [g[t] for t in traits]
    ct = OCG.cliquetree(net)
    spt = OCG.spanningtree_clusterlist(ct, OCG.default_rootcluster(ct, net))
    ocgb = oracle_setup(net, ct, model, tbl, g["taxa"])
    assert OC.calibrate(ocgb, [spt], verbose=False)[0]
    return net, model, tbl, g["taxa"], ocgb, spt


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_is_the_joint_posterior_of_the_dense_oracle(name):
    net, model, tbl, taxa, ocgb, spt = calibrated_case(name)
    nc = ocgb.nclusters
    records, dims, sepcl, soff, sidx = arrays_from_beliefs(ocgb.belief, nc, OB.scopeindex)
    D = sample_size(dims, nc)
    vn = variable_nodes(ocgb.belief, nc)
    assert D == len(vn) and D >= 6
    x, info = sample_posterior_ref(records, dims, sepcl, soff, sidx, spt[2], spt[3], unit_draws(D))
    assert info == 0 and x.shape == (1 + D, D)
    pm, pc = OD.posterior_node_moments(net, model, tbl, taxa)
    em, ec = law_errors(x, vn, model.dimension(), pm, pc)
    print(f"{name}: D = {D}, mean {em:.2e}, covariance {ec:.2e}")
    assert em <= 1e-8 and ec <= 1e-8
    # a variable held by several clusters: the same bits in all of them, in every draw
    first = {}
    shared = 0
    for k, nt in enumerate(vn):
        if nt in first:
            shared += 1
            assert np.array_equal(x[:, k], x[:, first[nt]]), nt
        else:
            first[nt] = k
    assert shared >= 1


def test_restatement_ignores_z_at_conditioned_positions_and_reports_failure():
    net, model, tbl, taxa, ocgb, spt = calibrated_case("level1_network_random_root")
    nc = ocgb.nclusters
    records, dims, sepcl, soff, sidx = arrays_from_beliefs(ocgb.belief, nc, OB.scopeindex)
    D = sample_size(dims, nc)
    rng = np.random.default_rng(3)
    z = rng.standard_normal((4, D))
    x, info = sample_posterior_ref(records, dims, sepcl, soff, sidx, spt[2], spt[3], z)
    assert info == 0
    # entries of z at S positions are ignored
    off = np.concatenate([[0], np.cumsum(dims[:nc])])
    z2 = z.copy()
    for pa, ch in zip(spt[2], spt[3]):
        k = next(k for k in range(len(sepcl)) if set(sepcl[k]) == {pa, ch})
        side = 0 if sepcl[k][0] == ch else 1
        z2[:, off[ch] + sidx[soff[2 * k + side]: soff[2 * k + side + 1]]] = 99.0
    x2, _ = sample_posterior_ref(records, dims, sepcl, soff, sidx, spt[2], spt[3], z2)
    assert np.array_equal(x, x2)
    # an indefinite R block: info names the cluster (1-based), everything is NaN
    c = int(spt[2][0])   # (the root: R is the whole cluster)
    J, h = records[c]
    bad = [(Jc.copy(), hc.copy()) for Jc, hc in records]
    bad[c] = (-np.eye(len(h)), h)
    xb, info = sample_posterior_ref(bad, dims, sepcl, soff, sidx, spt[2], spt[3], z)
    assert info == c + 1 and np.all(np.isnan(xb))
