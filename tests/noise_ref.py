"""Comparators for measurement error at the tips (pgbp_lg_set_tip_noise / set_tip_noise_lg), host side, shared by
test_tip_noise_cpu.py and test_gpu_tip_noise.py (tests only).

`NoisyTipModel` wraps any oracle model (a shift_ref.ShiftedModel included), as ShiftedModel does: it delegates the root prior
and returns branch_qwv(edge) = (q, w, v + E / gamma^2) on the FIRST parent edge of every noisy tip.  oracle.densemvn and the
generic hybrid factor weight an edge's v with gamma^2 (a tree edge: gamma = 1), so the conditional variance V_f of the tip's
family gains exactly E_f, below a hybrid node as on a tree edge.  The untouched oracle then states the noisy model twice:
densely (densemvn: loglik, posterior_node_moments, and through them loo_ref.dense_loo, impute_ref.dense_impute) and as belief
propagation (beliefs.assignfactors + calibration) from the GENERIC factors of oracle.models.EvolutionaryModel.

Also here, in numpy: the correction the device adds to a filled record (`correction`, `absorb_tip`), fill-then-correct
against the direct factor (`fill_then_correct_error`), and the family sweeps under noise (`family_statement`: gradient_lg with
dsigma_e, edge_gradient_lg and shift_scan_lg; loo_lg and impute_lg are stated densely by the wrapper)."""
import numpy as np

from edge_ref import edge_coefs
from oracle import densemvn as OD
from oracle import models as OM
from scan_ref import restricted_solve
from shift_ref import family_edge, family_nodes
from test_gradient_cpu import model_params


class NoisyTipModel(OM.EvolutionaryModel):
    """`model` with the variance E[edge.number] (p x p) added to the family of the tip below that edge; for a tip with
    several parent edges (a hybrid tip) the key is its first parent edge."""

    def __init__(self, model, noise):
        self.model = model
        self.p = model.dimension()
        self.noise = {int(k): np.asarray(v, float).reshape(self.p, self.p) for k, v in noise.items()}

    def dimension(self):
        return self.model.dimension()

    def rootpriormeanvector(self):
        return self.model.rootpriormeanvector()

    def rootpriorvariance(self):
        return self.model.rootpriorvariance()

    def isrootfixed(self):
        return self.model.isrootfixed()

    def factor_root(self):
        return self.model.factor_root()

    def branch_qwv(self, edge):
        q, w, v = self.model.branch_qwv(edge)
        E = self.noise.get(int(edge.number))
        if E is None:
            return q, w, v
        return q, w, np.atleast_2d(np.asarray(v, float)) + E / edge.gamma ** 2

    # a noisy family: the generic factor of branch_qwv; every other family: the wrapped model's own factor
    def factor_treeedge(self, edge):
        if int(edge.number) in self.noise:
            return OM.EvolutionaryModel.factor_treeedge(self, edge)
        return self.model.factor_treeedge(edge)

    def factor_hybridnode(self, pae):
        pae = list(pae)
        if any(int(e.number) in self.noise for e in pae):
            return OM.EvolutionaryModel.factor_hybridnode(self, pae)
        return self.model.factor_hybridnode(pae)


def tip_noise(scale, sigma_e, se2=None):
    """E_f = scale_f Sigma_e + diag(se2_f) of every listed tip: [n, p, p]."""
    sigma_e = np.atleast_2d(np.asarray(sigma_e, float))
    scale = np.asarray(scale, float).reshape(-1)
    E = scale[:, None, None] * sigma_e[None]
    if se2 is not None:
        E = E + np.stack([np.diag(s) for s in np.asarray(se2, float).reshape(len(scale), -1)])
    return E


def wrapper(net, ocgb, fam, model, families, E):
    """The noisy oracle model of a device case: families of the table given to lg_setup, E [n, p, p]."""
    return NoisyTipModel(model, {family_edge(net, ocgb, fam, int(f), 0).number: e for f, e in zip(families, E)})


def family_variance(fam, R, f, model="bm", alpha=None):
    """V_f = sum_k vc_k R[colour_k] of family f of the table (p x p)."""
    K = max(1, int(fam["max_parents"]))
    p = int(fam["p"])
    R = np.asarray(R, float).reshape(-1, p, p)
    V = np.zeros((p, p))
    for k in range(int(fam["n_parents"][f])):
        t, g, c = fam["length"][f * K + k], fam["gamma"][f * K + k], int(fam["color"][f * K + k])
        vc = g * g * (1.0 - np.exp(-2.0 * alpha * t)) if model == "ou" else g * g * t
        V += vc * R[c]
    return V


def draw_noise(fam, R, families, rng, lo=0.01, hi=100.0, model="bm", alpha=None, with_se2=True):
    """(scale [n], sigma_e [p, p], se2 [n, p] or None) such that diag(E_f) lies between `lo` and `hi` times diag(V_f) for
    every listed tip: sigma_e a random correlation pattern on the mean diagonal of the V_f, scale_f log-uniform, se2 filling
    up to a log-uniform target per trait."""
    return draw_noise_from_diag(np.array([np.diag(family_variance(fam, R, int(f), model, alpha)) for f in families]), rng, lo, hi,
                                with_se2)


def oracle_tip_variance(net, model, node):
    """V_f of the family of `node` from branch_qwv, as densemvn weights it: sum_k gamma_k^2 v_k."""
    return sum(e.gamma ** 2 * np.atleast_2d(np.asarray(model.branch_qwv(e)[2], float)) for e in net.parent_edges(node))


def draw_noise_from_diag(Vd, rng, lo=0.01, hi=100.0, with_se2=True):
    """draw_noise for the diagonals Vd [n, p] of the listed tips' V_f."""
    p = Vd.shape[1]
    A = rng.normal(size=(p, p))
    C = A @ A.T + p * np.eye(p)
    d = np.sqrt(np.diag(C))
    C = C / np.outer(d, d)
    base = np.sqrt(np.exp(np.mean(np.log(Vd), axis=0)))
    sigma_e = C * np.outer(base, base)
    ratio = np.max(np.diag(sigma_e)[None, :] / Vd, axis=1)           # per tip: the largest diag(Sigma_e) / diag(V)
    rmin = np.min(np.diag(sigma_e)[None, :] / Vd, axis=1)
    # scale_f so that scale_f diag(Sigma_e) stays inside [lo, hi / 2] x diag(V_f)
    top = np.minimum(0.5 * hi / ratio, hi)
    bot = lo / rmin
    assert np.all(bot < top), "the V_f of the listed tips are too unequal across traits for one Sigma_e"
    scale = np.exp(rng.uniform(np.log(bot), np.log(top)))
    se2 = None
    if with_se2:
        target = np.exp(rng.uniform(np.log(lo), np.log(hi), size=Vd.shape)) * Vd
        se2 = np.maximum(target - scale[:, None] * np.diag(sigma_e)[None, :], 0.0)
    E = tip_noise(scale, sigma_e, se2)
    r = np.array([np.diag(e) for e in E]) / Vd
    assert r.min() >= lo * (1 - 1e-12) and r.max() <= hi * (1 + 1e-12), (r.min(), r.max())
    return scale, sigma_e, se2


# ----------------------------------------------------------------------------- the correction of a filled record

def absorb_tip(phi, y, p):
    """A factor (h, J, g) over [child, parents] with the child's p traits fixed to y: the factor over the parents."""
    h, J, g = phi
    h, J = np.asarray(h, float), np.asarray(J, float)
    return h[p:] - J[p:, :p] @ y, J[p:, p:], float(g + h[:p] @ y - 0.5 * y @ J[:p, :p] @ y)


def correction(V, E, qs, zt):
    """What the device adds to the filled record of a noisy tip family with complete data: V, E (p x p), qs = [qc_k] the
    scalar coefficients of the in-scope parents (c_k = -qc_k), zt = z + delta (z = w - y as the fill forms it).
    D = -j E j' by solves, never as a difference of two inverses.  Returns (Delta h, Delta J, Delta g) over the parents."""
    jE = np.linalg.solve(V, E)
    D = -np.linalg.solve((V + E).T, jE.T).T      # -(j E) (V + E)^-1
    D = (D + D.T) / 2
    c = -np.asarray(qs, float)
    dJ = np.kron(np.outer(c, c), D)
    dh = np.concatenate([ck * (D @ zt) for ck in c])
    dg = -0.5 * float(zt @ D @ zt) - 0.5 * (np.linalg.slogdet(V + E)[1] - np.linalg.slogdet(V)[1])
    return dh, dJ, dg


def fill_then_correct_error(ratio, p=3, seed=0):
    """Relative error of fill + correction, j + D in double, against (V + E)^-1 formed in extended precision, |E| / |V| =
    ratio: (error of j + D, error of the direct double inverse -- the floor)."""
    rng = np.random.default_rng(seed)
    A, B = rng.normal(size=(p, p)), rng.normal(size=(p, p))
    V = A @ A.T / p + np.eye(p)
    E = B @ B.T / p + np.eye(p)
    E = E * (ratio * np.linalg.norm(V, 2) / np.linalg.norm(E, 2))
    ld = np.longdouble

    def inv_ld(M):   # Gauss-Jordan in extended precision
        n = M.shape[0]
        W = np.concatenate([M.astype(ld), np.eye(n, dtype=ld)], axis=1)
        for k in range(n):
            W[k] = W[k] / W[k, k]
            for i in range(n):
                if i != k:
                    W[i] = W[i] - W[i, k] * W[k]
        return W[:, n:]
    want = inv_ld(V + E)
    j = np.linalg.inv(V)
    D = -np.linalg.solve((V + E).T, np.linalg.solve(V, E).T).T
    got = j + D
    size = float(np.max(np.abs(want)))
    return float(np.max(np.abs(got.astype(ld) - want))) / size, float(np.max(np.abs(np.linalg.inv(V + E).astype(ld) - want))) / size


# ----------------------------------------------------------------------------- the family sweeps under noise

def family_statement(net, model, shifts, noise, scales, pm, pc, min_info=1e-8):
    """model: the PLAIN oracle model; shifts: {edge.number: s}; noise: {node index in preorder: E_f}, scales: {node index:
    scale_f}; pm / pc: posterior mean / covariance of all node states in preorder under the noisy (and shifted) model -- a
    noisy tip's state is its observation.  shift_ref.family_statement and scan_ref.family_scan with V + E_f for the noisy
    tips, and dsigma_e = sum_f scale_f G_V(f).  Rows = nodes in preorder."""
    pre = net.vec_node
    p = model.dimension()
    rates, root_color, mu, alpha, theta = model_params(model)
    pos = {id(n): i for i, n in enumerate(pre)}
    sl = lambda i: slice(i * p, (i + 1) * p)
    N = len(pre)
    K = max([1] + [len(net.parent_edges(n)) for n in pre])
    hetero = isinstance(model, OM.HeterogeneousBrownianMotion)
    ou = alpha is not None
    dR = np.zeros((len(rates), p, p))
    dsig = np.zeros((p, p))
    dmu, dth, dal = np.zeros(p), np.zeros(p), 0.0
    dlen, dgam = np.full((N, K), np.nan), np.full((N, K), np.nan)
    dshift = np.full((N, p), np.nan)
    jump, lr, ident = np.full((N, p), np.nan), np.full(N, np.nan), np.zeros((N, p), bool)
    edges = [[] for _ in range(N)]
    if root_color is not None:
        j = np.linalg.inv(rates[root_color])
        e = pm[sl(0)] - mu
        dR[root_color] += 0.5 * (j @ (pc[sl(0), sl(0)] + np.outer(e, e)) @ j - j)
        dmu += j @ e
        dshift[0] = j @ e
    for i in range(1, N):
        pes = net.parent_edges(pre[i])
        edges[i] = list(pes)
        co = [edge_coefs(alpha, ed.length, ed.gamma) for ed in pes]
        col = [model._c(ed) if hetero else 0 for ed in pes]
        pis = [pos[id(ed.parent)] for ed in pes]
        sk = [np.asarray(shifts.get(int(ed.number), np.zeros(p)), float) for ed in pes]
        V = sum(c[0][1] * rates[cc] for c, cc in zip(co, col))
        if i in noise:
            V = V + noise[i]
        j = np.linalg.inv(V)
        w = (sum(c[0][2] for c in co) * theta if ou else np.zeros(p)) + sum(ed.gamma * s for ed, s in zip(pes, sk))
        blocks = [(1.0, i)] + [(-c[0][0], pi) for c, pi in zip(co, pis)]
        e = sum(c * pm[sl(b)] for c, b in blocks) - w
        S = sum(ca * cb * pc[sl(a), sl(b)] for ca, a in blocks for cb, b in blocks)
        G = 0.5 * (j @ (S + np.outer(e, e)) @ j - j)
        gw = j @ e
        dshift[i] = gw
        if i in noise:
            dsig += scales[i] * G
        H = j - j @ S @ j
        kept, d, lr_i, _ = restricted_solve((H + H.T) / 2, gw, np.diag(j), min_info)
        jump[i], lr[i], ident[i] = d, lr_i, kept
        thg = float(theta @ gw) if ou else 0.0
        for k, (ed, pi) in enumerate(zip(pes, pis)):
            Erx = sum(c * pc[sl(b), sl(pi)] for c, b in blocks) + np.outer(e, pm[sl(pi)])
            gq = np.trace(j @ Erx)
            trGR = np.trace(G @ rates[col[k]])
            (qc, vc, wc), dt, dg = co[k]
            dlen[i, k] = dt[1] * trGR + dt[2] * thg + dt[0] * gq
            dgam[i, k] = dg[1] * trGR + dg[2] * thg + dg[0] * gq + float(sk[k] @ gw)
            dR[col[k]] += vc * G
            if pi == 0 and model.isrootfixed():
                dmu += qc * gw
            if ou:
                g_, t_ = ed.gamma, ed.length
                a = np.exp(-alpha * t_)
                dal += 2 * g_ * g_ * t_ * a * a * trGR + g_ * t_ * a * thg - g_ * t_ * a * gq
                dth += wc * gw
    return dict(dR=dR, dmu=dmu, dalpha=dal, dtheta=dth, dsigma_e=dsig, dlength=dlen, dgamma=dgam, dshift=dshift,
                jump=jump, lr=lr, identified=ident, edges=edges)


def dense_statement(net, model_w, model, shifts, noise, scales, tbl, taxa, min_info=1e-8):
    """family_statement on the dense posterior of the wrapper `model_w` (NoisyTipModel, around a ShiftedModel when shifts
    are set) -- proper or fixed root."""
    pm, pc = OD.posterior_node_moments(net, model_w, tbl, taxa)
    return family_statement(net, model, shifts, noise, scales, pm, pc, min_info)


def node_noise(ocgb, fam, families, E, scale):
    """({preorder node index: E_f}, {preorder node index: scale_f}) of the listed families of the table."""
    nodes = family_nodes(ocgb, fam)
    return {nodes[int(f)]: e for f, e in zip(families, E)}, {nodes[int(f)]: float(s) for f, s in zip(families, scale)}


# ----------------------------------------------------------------------------- the workaround: a pendant node per noisy tip

def pendant_case(tree, R, sigma_e, mu, v, tips, scale):
    """What a user had to do before: the oracle TREE with a second node hung under every tip of `tips` (names) on an edge of
    length scale_f whose rate colour is Sigma_e.  The new leaf keeps the tip's name (and so its data row), the old tip becomes
    the internal node <name>_x.  Returns (tree, HeterogeneousBrownianMotion with the rates [R, Sigma_e])."""
    from impute_ref import tree_newick
    from oracle import network as ON
    nwk = tree_newick(tree)
    for name, s in zip(tips, scale):
        for lead in "(,":
            nwk = nwk.replace(f"{lead}{name}:", f"{lead}({name}:{float(s)!r}){name}_x:")
    net = ON.read_newick(nwk)
    colors = {e.number: 2 for e in net.edges if e.child.leaf and e.child.name in set(tips)}
    assert len(colors) == len(tips)
    return net, OM.HeterogeneousBrownianMotion([R, sigma_e], colors, mu, v)
