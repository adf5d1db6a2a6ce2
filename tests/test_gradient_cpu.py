"""The analytic gradient of the log-likelihood, host side (no GPU):

* `_BMTransform.pullback` (optimize.py) against Richardson-extrapolated central differences;
* `family_gradient`: a numpy statement of Fisher's identity d loglik / d theta = sum_f E[d log phi_f / d theta | data] over
  the node families, the expectations taken from the DENSE oracle (oracle/densemvn.py: posterior_node_moments, which shares
  no code with message passing), against Richardson central differences of densemvn.loglik.  The GPU tests
  (test_gpu_gradient.py) compare the device sweep with this statement, so the formulas are pinned to the independent oracle
  here first.  Measured: 7.6e-12 (dR), 4.8e-11 (dmu) for the BM case, <= 1.6e-11 for the OU case; asserted at 1e-8.
"""
import numpy as np
import pytest

from oracle import densemvn as OD
from oracle import models as OM
from oracle import network as ON


# ----------------------------------------------------------------------------- the numpy statement

def model_params(model):
    """(rates [list of p x p], root-prior colour or None, mu, alpha or None, theta or None) as the device's rate table
    holds them (helpers.lg_inputs_from_oracle): an OU model's rate is its stationary variance."""
    if isinstance(model, OM.HeterogeneousBrownianMotion):
        rates = [np.array(r, float) for r in model.rates]
    elif isinstance(model, OM.UnivariateOrnsteinUhlenbeck):
        rates = [np.array([[model.gamma2]])]
    else:
        rates = [np.array(model.R, float)]
    v = np.atleast_2d(np.asarray(model.rootpriorvariance(), float))
    root_color = None
    if not model.isrootfixed() and not np.any(np.isinf(np.diag(v))):
        root_color = len(rates)
        rates = rates + [v.copy()]
    ou = isinstance(model, OM.UnivariateOrnsteinUhlenbeck)
    return rates, root_color, np.array(model.rootpriormeanvector(), float), (model.alpha if ou else None), \
        (np.array([model.theta]) if ou else None)


def model_with(model, rates, mu, alpha=None, theta=None):
    """The same kind of model with other parameter values (rates as model_params lists them)."""
    rates = [np.array(r, float) for r in rates]
    v = np.atleast_2d(np.asarray(model.rootpriorvariance(), float))
    proper = not model.isrootfixed() and not np.any(np.isinf(np.diag(v)))
    vv = rates[-1] if proper else (None if model.isrootfixed() else v)
    body = rates[:-1] if proper else rates
    if isinstance(model, OM.HeterogeneousBrownianMotion):
        return OM.HeterogeneousBrownianMotion(body, model.colors, mu, vv)
    if isinstance(model, OM.UnivariateOrnsteinUhlenbeck):
        g2 = float(body[0][0, 0])
        return OM.UnivariateOrnsteinUhlenbeck(2.0 * alpha * g2, alpha, float(np.ravel(theta)[0]), float(np.ravel(mu)[0]),
                                              None if vv is None else float(vv[0, 0]))
    return OM.MvFullBrownianMotion(body[0], mu, vv)


def family_gradient(net, model, pm, pc):
    """Section "the mathematics" of the gradient: per family r = x_child - sum_k q_k x_k - w, e = E[r], M = Cov(r) + e e',
    G_V = (j M j - j) / 2, g_w = j e, g_qk = E[r' j x_k]; pm / pc: posterior mean / covariance of ALL node states in
    preorder (a fixed root, an observed tip value: variance 0).  Returns dict(dR [n_rates, p, p], dmu, dalpha, dtheta)."""
    pre = net.vec_node
    p = model.dimension()
    rates, root_color, mu, alpha, theta = model_params(model)
    pos = {id(n): i for i, n in enumerate(pre)}
    sl = lambda i: slice(i * p, (i + 1) * p)
    dR = np.zeros((len(rates), p, p))
    dmu, dth, dal = np.zeros(p), np.zeros(p), 0.0
    ou = alpha is not None
    hetero = isinstance(model, OM.HeterogeneousBrownianMotion)
    if root_color is not None:
        j = np.linalg.inv(rates[root_color])
        e = pm[sl(0)] - mu
        M = pc[sl(0), sl(0)] + np.outer(e, e)
        dR[root_color] += 0.5 * (j @ M @ j - j)
        dmu += j @ e
    for i in range(1, len(pre)):
        pes = net.parent_edges(pre[i])
        qc, vc, wc, dqc, dvc, dwc, col, pis = [], [], [], [], [], [], [], []
        for ed in pes:
            g, t = ed.gamma, ed.length
            if ou:
                a = np.exp(-alpha * t)
                qc.append(g * a); vc.append(g * g * (1 - a * a)); wc.append(g * (1 - a))
                dqc.append(-g * t * a); dvc.append(2 * g * g * t * a * a); dwc.append(g * t * a)
            else:
                qc.append(g); vc.append(g * g * t); wc.append(0.0)
                dqc.append(0.0); dvc.append(0.0); dwc.append(0.0)
            col.append(model._c(ed) if hetero else 0)
            pis.append(pos[id(ed.parent)])
        V = sum(v * rates[c] for v, c in zip(vc, col))
        j = np.linalg.inv(V)
        w = sum(wc) * theta if ou else np.zeros(p)
        blocks = [(1.0, i)] + [(-q, pi) for q, pi in zip(qc, pis)]
        e = sum(c * pm[sl(b)] for c, b in blocks) - w
        S = sum(ca * cb * pc[sl(a), sl(b)] for ca, a in blocks for cb, b in blocks)
        M = S + np.outer(e, e)
        G = 0.5 * (j @ M @ j - j)
        gw = j @ e
        for k, pi in enumerate(pis):
            dR[col[k]] += vc[k] * G
            if pi == 0 and model.isrootfixed():
                dmu += qc[k] * gw
            if ou:
                Erx = sum(c * pc[sl(b), sl(pi)] for c, b in blocks) + np.outer(e, pm[sl(pi)])
                gq = np.trace(j @ Erx)
                dal += dvc[k] * np.trace(G @ rates[col[k]]) + dwc[k] * float(theta @ gw) + dqc[k] * gq
        if ou:
            dth += sum(wc) * gw
    return dict(dR=dR, dmu=dmu, dalpha=dal, dtheta=dth)


def dense_gradient(net, model, tbl, taxa):
    """family_gradient on the dense oracle's posterior moments (proper or fixed root)."""
    pm, pc = OD.posterior_node_moments(net, model, tbl, taxa)
    return family_gradient(net, model, pm, pc)


# ----------------------------------------------------------------------------- finite differences of the dense likelihood

def richardson(f, h):
    """Central difference of f at 0 with steps h and h / 2, extrapolated: error O(h^4)."""
    d1 = (f(h) - f(-h)) / (2 * h)
    d2 = (f(h / 2) - f(-h / 2)) / h
    return (4 * d2 - d1) / 3


def fd_gradient(net, model, tbl, taxa, h=1e-3):
    """The same dict as family_gradient from Richardson central differences (steps h, h / 2) of densemvn.loglik; dR[c][a, b]
    is the derivative along (E_ab + E_ba) / 2."""
    rates, root_color, mu, alpha, theta = model_params(model)
    p = model.dimension()

    def ll(rates_=rates, mu_=mu, alpha_=alpha, theta_=theta):
        return OD.loglik(net, model_with(model, rates_, mu_, alpha_, theta_), tbl, taxa)
    dR = np.zeros((len(rates), p, p))
    for c in range(len(rates)):
        for a in range(p):
            for b in range(a, p):
                E = np.zeros((p, p))
                E[a, b] += 0.5
                E[b, a] += 0.5

                def f(s, c=c, E=E):
                    rr = [r.copy() for r in rates]
                    rr[c] = rr[c] + s * E
                    return ll(rates_=rr)
                dR[c, a, b] = dR[c, b, a] = richardson(f, h)
    improper = np.any(np.isinf(np.diag(np.atleast_2d(np.asarray(model.rootpriorvariance(), float)))))
    dmu = np.zeros(p)
    if not improper:
        for a in range(p):
            dmu[a] = richardson(lambda s, a=a: ll(mu_=mu + s * np.eye(p)[a]), h)
    out = dict(dR=dR, dmu=dmu, dalpha=0.0, dtheta=np.zeros(p))
    if alpha is not None:
        out["dalpha"] = richardson(lambda s: ll(alpha_=alpha + s), h)
        out["dtheta"] = np.array([richardson(lambda s: ll(theta_=theta + s), h)])
    return out


def rel_block(got, want):
    """max |got - want| relative to the largest entry of the block."""
    got, want = np.asarray(got, float), np.asarray(want, float)
    return float(np.max(np.abs(got - want)) / max(np.max(np.abs(want)), 1e-300))


# ----------------------------------------------------------------------------- tests

@pytest.mark.parametrize("diagonal", [False, True])
@pytest.mark.parametrize("p", [1, 2, 5])
def test_pullback_against_central_differences(p, diagonal):
    """pullback = the gradient in theta of f(back(theta)) for a smooth scalar f of (R, mu); 1e-8 relative to the largest
    entry (Richardson steps 1e-3 / 5e-4: error O(h^4))."""
    from pgbp_amd.optimize import _BMTransform
    rng = np.random.default_rng(100 + p)
    tf = _BMTransform(p, diagonal)
    A = rng.normal(size=(p, p))
    C = rng.normal(size=(p, p)); C = C + C.T
    b = rng.normal(size=p)

    def f(R, mu):
        return float(np.sum(C * R) + 0.3 * np.sum((A @ R) ** 2) + np.linalg.slogdet(R)[1] + b @ mu + 0.5 * mu @ R @ mu)

    def df(R, mu):   # symmetric gradient in R, gradient in mu
        g = C + 0.6 * (A.T @ A @ R) + np.linalg.inv(R) + 0.5 * np.outer(mu, mu)
        return (g + g.T) / 2, b + R @ mu
    B = rng.normal(size=(p, p))
    R0 = np.diag(rng.uniform(0.5, 2, p)) if diagonal else B @ B.T / p + np.eye(p)
    th = tf.forward(R0, rng.normal(size=p))
    R, mu = tf.back(th)
    got = tf.pullback(th, *df(R, mu))
    want = np.array([richardson(lambda s, i=i: f(*tf.back(th + s * np.eye(len(th))[i])), 1e-3) for i in range(len(th))])
    err = rel_block(got, want)
    print(f"p={p} diagonal={diagonal}: pullback vs Richardson {err:.2e}")
    assert got.shape == th.shape and err <= 1e-8


def _case(which):
    rng = np.random.default_rng(7)
    net = ON.random_network(30, 6, rng)
    taxa = net.tip_names
    if which == "bm":
        p = 2
        A = rng.normal(size=(p, p))
        B = rng.normal(size=(p, p))
        model = OM.MvFullBrownianMotion(A @ A.T / p + np.eye(p), rng.normal(size=p), B @ B.T / p + 0.5 * np.eye(p))
    else:
        p = 1
        model = OM.UnivariateOrnsteinUhlenbeck(rng.uniform(0.5, 2), rng.uniform(0.1, 1), rng.normal(), rng.normal(), 0.8)
    tbl = [list(rng.normal(size=len(taxa))) for _ in range(p)]
    return net, model, tbl, taxa


@pytest.mark.parametrize("which", ["bm", "ou"])
def test_fisher_identity_on_the_dense_oracle(which):
    """Random network, 30 tips, 6 hybrid nodes, proper root prior: full BM (p = 2) and the univariate OU; every block of
    the gradient within 1e-8 of the Richardson central differences (1e-3, 5e-4) of densemvn.loglik."""
    net, model, tbl, taxa = _case(which)
    got = dense_gradient(net, model, tbl, taxa)
    want = fd_gradient(net, model, tbl, taxa)
    names = ["dR", "dmu"] + (["dalpha", "dtheta"] if which == "ou" else [])
    for k in names:
        err = rel_block(got[k], want[k])
        print(f"{which} {k}: {err:.2e}")
        assert err <= 1e-8, (k, got[k], want[k])
    for c in range(got["dR"].shape[0]):
        assert rel_block(got["dR"][c], want["dR"][c]) <= 1e-8


def _more_cases():
    rng = np.random.default_rng(17)
    net = ON.random_network(16, 4, rng)
    taxa = net.tip_names
    A = rng.normal(size=(2, 2))
    R = A @ A.T / 2 + np.eye(2)
    full = [list(rng.normal(size=len(taxa))) for _ in range(2)]
    colors = {e.number: 1 + int(rng.integers(3)) for e in net.edges}
    rates = [R * s for s in (0.5, 1.0, 2.5)]
    holes = [[None if rng.random() < 0.3 else v for v in col] for col in full]
    for r in range(len(taxa)):
        if holes[0][r] is None and holes[1][r] is None:
            holes[0][r] = full[0][r]
    yield "bm_fixed_root", net, OM.MvFullBrownianMotion(R, rng.normal(size=2)), full, taxa
    yield "hetero3_fixed_root", net, OM.HeterogeneousBrownianMotion(rates, colors, rng.normal(size=2)), full, taxa
    yield "hetero3_random_root", net, OM.HeterogeneousBrownianMotion(rates, colors, rng.normal(size=2), 0.7 * np.eye(2)), full, taxa
    yield "missing_fixed_root", net, OM.MvFullBrownianMotion(R, rng.normal(size=2)), holes, taxa
    yield "missing_random_root", net, OM.MvFullBrownianMotion(R, rng.normal(size=2), 0.7 * np.eye(2)), holes, taxa
    yield "ou_fixed_root", net, OM.UnivariateOrnsteinUhlenbeck(1.3, 0.4, 0.2, -0.5, 0.0), full[:1], taxa


@pytest.mark.parametrize("case", list(_more_cases()), ids=lambda c: c[0])
def test_fisher_identity_other_branches_of_the_statement(case):
    """The branches of family_gradient the two cases above do not reach -- the fixed root's dmu, several colours, missing tip
    values, the fixed-root OU -- against the same Richardson central differences of densemvn.loglik, 1e-8 per block and per
    colour (measured <= 4e-10)."""
    name, net, model, tbl, taxa = case
    got = dense_gradient(net, model, tbl, taxa)
    want = fd_gradient(net, model, tbl, taxa)
    for k in ("dR", "dmu", "dalpha", "dtheta"):
        if not np.any(np.atleast_1d(want[k])) and not np.any(np.atleast_1d(got[k])):
            continue
        parts = zip(got[k], want[k]) if k == "dR" else [(got[k], want[k])]
        for c, (a, b) in enumerate(parts):
            err = rel_block(a, b)
            print(f"{name} {k}[{c}]: {err:.2e}")
            assert err <= 1e-8, (name, k, c, a, b)
