"""The adjoint and forward recurrences of pgbp_posterior_cov, host side (no GPU): tests/cov_ref.py, their plain numpy
restatement, against the DENSE oracle (oracle/densemvn.py: posterior_node_moments) and against the explicit map A of the
sampler's restatement (tests/sample_ref.py), on the four calibrated cases of test_sample_cpu.py.

With c = I_D (D = the sample size) row a of k is Cov(x, x_a | data): compared with the oracle's posterior covariance on EVERY
pair of entries, across clusters too; row a of w is row a of A, compared with A = X[1:] - X[0] of the sampler's restatement at
z = [0; I_D]; and w w' is the same covariance again.  Bound: 1e-8 relative to the largest entry of the reference (the
project's parity bound).  Measured over the four cases: k <= 4.0e-16, w against A <= 5.0e-16, w w' <= 4.0e-16, a column on
another copy of a variable 0 (the same values)."""
import numpy as np
import pytest

from cov_ref import posterior_cov_ref, s_positions
from oracle import beliefs as OB
from oracle import densemvn as OD
from sample_ref import arrays_from_beliefs, sample_posterior_ref, sample_size, unit_draws, variable_nodes
from test_sample_cpu import CASES, calibrated_case


def _rel(got, want):
    return float(np.max(np.abs(got - want)) / max(np.max(np.abs(want)), 1e-300))


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request):
    """the arrays of one calibrated case, the dense posterior covariance on its entries, and the restatement at c = I_D"""
    net, model, tbl, taxa, ocgb, spt = calibrated_case(request.param)
    nc = ocgb.nclusters
    arrays = arrays_from_beliefs(ocgb.belief, nc, OB.scopeindex)
    D = sample_size(arrays[1], nc)
    vn = variable_nodes(ocgb.belief, nc)
    p = model.dimension()
    _, pc = OD.posterior_node_moments(net, model, tbl, taxa)
    flat = np.array([n * p + t for n, t in vn], dtype=int)
    w, k, info = posterior_cov_ref(*arrays, spt[2], spt[3], np.eye(D))
    assert info == 0 and w.shape == k.shape == (D, D)
    return dict(name=request.param, arrays=arrays, spt=spt, D=D, vn=vn, nc=nc, dense=pc[np.ix_(flat, flat)], w=w, k=k)


def test_k_is_the_dense_posterior_covariance_on_every_pair(case):
    e = _rel(case["k"], case["dense"])
    print(f"{case['name']}: D = {case['D']}, k against the dense covariance {e:.2e}")
    assert e <= 1e-8


def test_w_is_the_transpose_of_the_samplers_map(case):
    D = case["D"]
    x, info = sample_posterior_ref(*case["arrays"], case["spt"][2], case["spt"][3], unit_draws(D))
    assert info == 0
    A = (x[1:] - x[0]).T          # A[entry, z]: x = m + A z
    e = _rel(case["w"], A)
    print(f"{case['name']}: w against A {e:.2e}")
    assert e <= 1e-8


def test_w_w_transposed_is_the_dense_posterior_covariance(case):
    e = _rel(case["w"] @ case["w"].T, case["dense"])
    print(f"{case['name']}: w w' against the dense covariance {e:.2e}")
    assert e <= 1e-8


def test_w_is_exactly_zero_at_conditioned_positions(case):
    records, dims, sepcl, soff, sidx = case["arrays"]
    S = s_positions(dims, sepcl, soff, sidx, case["spt"][2], case["spt"][3], case["nc"])
    assert len(S) >= 1
    assert np.all(case["w"][:, S] == 0.0)
    rng = np.random.default_rng(4)
    w, _, _ = posterior_cov_ref(*case["arrays"], case["spt"][2], case["spt"][3], rng.standard_normal((3, case["D"])))
    assert np.all(w[:, S] == 0.0) and np.any(w != 0.0)


def test_weight_on_another_copy_of_a_variable_gives_the_same_k(case):
    first, worst, shared = {}, 0.0, 0
    scale = float(np.max(np.abs(case["k"])))
    for a, nt in enumerate(case["vn"]):
        if nt in first:
            shared += 1
            worst = max(worst, float(np.max(np.abs(case["k"][a] - case["k"][first[nt]]))) / scale)
        else:
            first[nt] = a
    print(f"{case['name']}: {shared} further copies, k of a copy against k of the first {worst:.2e}")
    assert shared >= 1 and worst <= 1e-8


def test_indefinite_block_gives_the_samplers_info():
    net, model, tbl, taxa, ocgb, spt = calibrated_case("level1_network_random_root")
    nc = ocgb.nclusters
    arrays = arrays_from_beliefs(ocgb.belief, nc, OB.scopeindex)
    D = sample_size(arrays[1], nc)
    named = 0
    for cl in range(nc):      # (a cluster whose R is empty has nothing to factor: both report 0)
        bad = [(J.copy(), h.copy()) for J, h in arrays[0]]
        bad[cl] = (-np.eye(len(bad[cl][1])), bad[cl][1])
        _, sinfo = sample_posterior_ref(bad, *arrays[1:], spt[2], spt[3], np.zeros((1, D)))
        w, k, info = posterior_cov_ref(bad, *arrays[1:], spt[2], spt[3], np.eye(D)[:2])
        assert info == sinfo and info in (0, cl + 1)
        if info:
            named += 1
            assert np.all(np.isnan(w)) and np.all(np.isnan(k))
    assert named >= 2
