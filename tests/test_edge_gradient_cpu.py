"""Per-edge derivatives of the log-likelihood, host side (no GPU): edge_ref.family_edge_gradient -- the numpy statement of
d loglik / d (edge length, inheritance, mean shift) per node family, fed from the DENSE oracle's posterior moments --
against Richardson central differences (steps 1e-3 and 5e-4, relative to the perturbed value) of densemvn.loglik.  The GPU
tests (test_gpu_edge_gradient.py) compare the device sweep with this statement, so the formulas are pinned to the
independent oracle here first.  Asserted at 1e-8 relative to the largest entry of each block (dlength, dgamma, dshift), the
bound of test_gradient_cpu; the measured figures are printed (largest over the eight cases: 4.2e-11)."""
import numpy as np
import pytest

from edge_ref import dense_edge_gradient, fd_edge_gradient, rel_block_nan
from oracle import densemvn as OD
from test_gradient_cpu import _case, _more_cases, dense_gradient, model_params, rel_block, richardson

BLOCKS = ("dlength", "dgamma", "dshift")


def _cases():
    for which in ("bm", "ou"):
        yield (which + "_random_root",) + _case(which)
    yield from _more_cases()


CASES = list(_cases())
_REF = {}


def _ref(case):
    """The dense statement of a case, computed once and shared."""
    name, net, model, tbl, taxa = case
    if name not in _REF:
        _REF[name] = dense_edge_gradient(net, model, tbl, taxa)
    return _REF[name]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_edge_statement_against_the_dense_oracle(case):
    """Every edge's length and (free) inheritance, and the mean shift of every family, within 1e-8 of the block's largest
    entry of the Richardson central differences of densemvn.loglik: fixed and random roots, three colours, missing values,
    the univariate OU."""
    name, net, model, tbl, taxa = case
    got = _ref(case)
    want = fd_edge_gradient(net, model, tbl, taxa)
    for k in BLOCKS:
        err = rel_block_nan(got[k], want[k])
        print(f"{name} {k}: {err:.2e}")
        assert err <= 1e-8, (name, k)


@pytest.mark.parametrize("case", [CASES[0], CASES[1]], ids=lambda c: c[0])
def test_constrained_inheritance_of_a_hybrid(case):
    """d/d gamma_major at gamma_minor = 1 - gamma_major is dgamma[major] - dgamma[minor]: against moving both inheritances of
    every hybrid node together."""
    name, net, model, tbl, taxa = case
    got = _ref(case)
    n_hyb = 0
    for i, eds in enumerate(got["edges"]):
        if len(eds) != 2:
            continue
        n_hyb += 1
        a, b = eds
        ga, gb = a.gamma, b.gamma

        def f(s):
            a.gamma, b.gamma = ga + s, gb - s
            try:
                return OD.loglik(net, model, tbl, taxa)
            finally:
                a.gamma, b.gamma = ga, gb
        want = richardson(f, 1e-3 * ga)
        have = got["dgamma"][i, 0] - got["dgamma"][i, 1]
        scale = np.nanmax(np.abs(got["dgamma"]))
        print(f"{name} hybrid {i}: constrained {have:.6e}, finite differences {want:.6e}")
        assert abs(have - want) <= 1e-8 * scale
    assert n_hyb == 6


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_conventions_and_identities(case):
    """NaN where there is no edge (the root row, k = 1 of a tree node), finite elsewhere; the root prior's row of dshift is
    dmu for a random root; sum over the families whose parent is the fixed root of qc_k dshift = dmu; sum over the families of
    (sum_k wc_k) dshift = dtheta (family_gradient of test_gradient_cpu)."""
    name, net, model, tbl, taxa = case
    got = _ref(case)
    grad = dense_gradient(net, model, tbl, taxa)
    N, K = got["dlength"].shape
    assert K == 2 and np.isnan(got["dlength"][0]).all() and np.isnan(got["dgamma"][0]).all()
    for i in range(1, N):
        n = len(got["edges"][i])
        for k in range(K):
            assert np.isnan(got["dlength"][i, k]) == (k >= n) and np.isnan(got["dgamma"][i, k]) == (k >= n)
        assert np.isfinite(got["dshift"][i]).all()
    root_color, alpha = model_params(model)[1], model_params(model)[3]
    if root_color is not None:
        assert rel_block(got["dshift"][0], grad["dmu"]) <= 1e-12
    else:
        assert np.isnan(got["dshift"][0]).all()
        pos = {id(n): i for i, n in enumerate(net.vec_node)}
        dmu = sum(got["qc"][i, k] * got["dshift"][i] for i in range(1, N) for k, ed in enumerate(got["edges"][i])
                  if pos[id(ed.parent)] == 0)
        assert rel_block(dmu, grad["dmu"]) <= 1e-12
    if alpha is not None:
        dth = sum(got["wc"][i].sum() * got["dshift"][i] for i in range(1, N))
        assert rel_block(dth, grad["dtheta"]) <= 1e-12
    # the sign: lengthening an edge by dt adds dt * dlength to the log-likelihood (first order)
    i = max(range(1, N), key=lambda i: abs(got["dlength"][i, 0]))
    ed = got["edges"][i][0]
    base = OD.loglik(net, model, tbl, taxa)
    keep = ed.length
    ed.length = keep * (1 + 1e-4)
    try:
        moved = OD.loglik(net, model, tbl, taxa)
    finally:
        ed.length = keep
    assert np.sign(moved - base) == np.sign(got["dlength"][i, 0])
