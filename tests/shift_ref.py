"""Comparators for mean shifts on edges (pgbp_lg_set_shifts / set_shifts_lg / fit_shifts_lg), host side, shared by
test_shift_cpu.py and test_gpu_shifts.py (tests only).

`ShiftedModel` wraps any oracle model: it delegates the root prior and returns branch_qwv(edge) = (q, w + s[edge], v); the
factors come from the GENERIC factor_treeedge / factor_hybridnode of oracle.models.EvolutionaryModel.  The untouched oracle
then states the shifted model twice: densely (densemvn) and as belief propagation (beliefs.assignfactors + calibration).
Both weight the displacement of an edge with its gamma, as the device does.

`family_statement` is the numpy statement of the family sweeps under shifts (test_gradient_cpu.family_gradient and
edge_ref.family_edge_gradient with the offset w + d, d = sum_k gamma_k s_k, and the new term of dgamma); `gls_fit` the dense
generalised-least-squares statement of the fit."""
import numpy as np

from edge_ref import edge_coefs, shift_transfer
from oracle import densemvn as OD
from oracle import models as OM
from test_gradient_cpu import model_params


class ShiftedModel(OM.EvolutionaryModel):
    """`model` with a displacement shifts[edge.number] (a p-vector) of the child's conditional mean on the listed edges."""

    def __init__(self, model, shifts):
        self.model = model
        self.p = model.dimension()
        self.shifts = {int(k): np.asarray(v, float).reshape(self.p) for k, v in shifts.items()}

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
        return q, np.asarray(w, float).reshape(self.p) + self.shifts.get(int(edge.number), np.zeros(self.p)), v

    # The factors.  The generic factor_treeedge / factor_hybridnode of EvolutionaryModel (inherited: `generic_factor`) state
    # the shifted factor from branch_qwv alone, but they invert V themselves, and under MISSING DATA the oracle's marginalize
    # tests a block for exact zeros (src/beliefupdates.jl:62-66) that only the models' own J = [j -j; -j j] leaves exact.  So
    # the factor handed to belief propagation is the wrapped model's own factor plus the shift's terms, by the linearity of
    # factor_from_qwj in w: h += [j d; -q' j d], g -= d' j w + d' j d / 2.  test_shift_cpu.py pins both forms to each other
    # where the generic one works, and belief propagation of this wrapper to densemvn, which sees branch_qwv only.
    def generic_factor(self, pae):
        pae = list(pae)
        if len(pae) == 1:
            return OM.EvolutionaryModel.factor_treeedge(self, pae[0])
        return OM.EvolutionaryModel.factor_hybridnode(self, pae)

    def _shifted(self, phi, pae, tree):
        h, J, g = phi
        p = self.p
        qs, w, d = [], np.zeros(p), np.zeros(p)
        for e in pae:
            q, we, _ = self.model.branch_qwv(e)
            c = 1.0 if tree else e.gamma
            qs.append(c * np.atleast_2d(q))
            w = w + c * np.asarray(we, float).reshape(p)
            d = d + c * self.shifts.get(int(e.number), np.zeros(p))
        j = np.asarray(J, float)[:p, :p]
        jd = j @ d
        h = np.asarray(h, float) + np.concatenate([jd] + [-q.T @ jd for q in qs])
        return h, J, float(g - d @ j @ w - 0.5 * d @ jd)

    def factor_treeedge(self, edge):
        return self._shifted(self.model.factor_treeedge(edge), [edge], True)

    def factor_hybridnode(self, pae):
        return self._shifted(self.model.factor_hybridnode(pae), list(pae), False)


# ----------------------------------------------------------------------------- the family table and the oracle's edges

def family_nodes(ocgb, fam):
    """Preorder node index of every family of the table lg_inputs_from_oracle builds (the root's family only when it has a
    prior factor)."""
    n = len(ocgb.node2family)
    skip = n - len(fam["cluster"])
    assert skip in (0, 1)
    return list(range(skip, n))

def family_edge(net, ocgb, fam, f, k):
    """The oracle Edge of parent edge k of family f."""
    pre = net.vec_node
    i = family_nodes(ocgb, fam)[f]
    p1 = ocgb.node2family[i][1 + k]
    return next(e for e in pre[p1 - 1].edges if e.child is pre[i])


def family_of_edge(net, ocgb, fam, ed):
    """(f, k) of an oracle Edge."""
    pre = net.vec_node
    nodes = family_nodes(ocgb, fam)
    i = next(j for j, n in enumerate(pre) if n is ed.child)
    k = next(q for q, p1 in enumerate(ocgb.node2family[i][1:]) if pre[p1 - 1] is ed.parent)
    return nodes.index(i), k


def tips_below(net, model, c):
    """Preorder indices of the tips that a displacement of node c reaches."""
    tau = shift_transfer(net, model, c)
    return [i for i, n in enumerate(net.vec_node) if n.leaf and tau[i] != 0.0]


def fit_edges(net, model):
    """The edge set of the fit tests: three tree edges into internal nodes with at least three tips below (the first, the
    middle and the last such node in preorder) and one hybrid edge (the first parent edge of the first hybrid node)."""
    pre = net.vec_node
    cand = [i for i in range(1, len(pre)) if not pre[i].leaf and len(net.parent_edges(pre[i])) == 1
            and len(tips_below(net, model, i)) >= 3]
    pick = [cand[0], cand[len(cand) // 2], cand[-1]]
    assert len(set(pick)) == 3
    out = [net.parent_edges(pre[i])[0] for i in pick]
    hyb = [i for i in range(1, len(pre)) if len(net.parent_edges(pre[i])) >= 2]
    if hyb:
        out.append(net.parent_edges(pre[hyb[0]])[0])
    return out


# ----------------------------------------------------------------------------- the sweeps, restated with the offset d

def family_statement(net, model, shifts, pm, pc):
    """model: the PLAIN oracle model; shifts: {edge.number: s}; pm / pc: posterior mean / covariance of all node states in
    preorder under the SHIFTED model (densemvn.posterior_node_moments of the wrapper).  Per family r = x_child - sum_k qc_k x_k
    - w - d, d = sum_k gamma_k s_k; e, M, G_V, g_w, g_qk as in test_gradient_cpu.family_gradient.  Returns the entries of
    family_gradient (dR, dmu, dalpha, dtheta) and of edge_ref.family_edge_gradient (dlength, dgamma, dshift, edges: rows =
    nodes in preorder), with dgamma[i, k] += s_k' g_w."""
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
    dmu, dth, dal = np.zeros(p), np.zeros(p), 0.0
    dlen, dgam = np.full((N, K), np.nan), np.full((N, K), np.nan)
    dshift = np.full((N, p), np.nan)
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
        j = np.linalg.inv(V)
        w = (sum(c[0][2] for c in co) * theta if ou else np.zeros(p)) + sum(ed.gamma * s for ed, s in zip(pes, sk))
        blocks = [(1.0, i)] + [(-c[0][0], pi) for c, pi in zip(co, pis)]
        e = sum(c * pm[sl(b)] for c, b in blocks) - w
        S = sum(ca * cb * pc[sl(a), sl(b)] for ca, a in blocks for cb, b in blocks)
        G = 0.5 * (j @ (S + np.outer(e, e)) @ j - j)
        gw = j @ e
        dshift[i] = gw
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
    return dict(dR=dR, dmu=dmu, dalpha=dal, dtheta=dth, dlength=dlen, dgamma=dgam, dshift=dshift, edges=edges)


def dense_statement(net, model, shifts, tbl, taxa):
    pm, pc = OD.posterior_node_moments(net, ShiftedModel(model, shifts), tbl, taxa)
    return family_statement(net, model, shifts, pm, pc)


def device_layout(st, net, ocgb, fam):
    """dlength / dgamma / dshift of family_statement (rows = nodes, columns = net.parent_edges order) as the device returns
    them: rows = families, columns = the table's per-parent order."""
    nodes = family_nodes(ocgb, fam)
    K = max(1, int(fam["max_parents"]))
    out = {k: np.full((len(nodes), K), np.nan) for k in ("dlength", "dgamma")}
    out["dshift"] = st["dshift"][nodes].copy()
    for f, i in enumerate(nodes):
        for k in range(int(fam["n_parents"][f])):
            ed = family_edge(net, ocgb, fam, f, k)
            kk = next(q for q, e2 in enumerate(st["edges"][i]) if e2 is ed)
            out["dlength"][f, k] = st["dlength"][i, kk]
            out["dgamma"][f, k] = st["dgamma"][i, kk]
    return out


# ----------------------------------------------------------------------------- the fit, densely

def gls_fit(net, model, tbl, taxa, edges):
    """Dense GLS of the shifts on `edges` (oracle Edge objects) at the model's parameters, fixed or proper random root:
    X = the offsets of a unit shift at the observed tip entries (column = edge-major, trait-minor), S = the covariance of the
    observed tip entries, m0 their mean without shifts.  Returns (shat [n, p], H [n p, n p], loglik at shat)."""
    pre = net.vec_node
    p = model.dimension()
    m0, cov, _ = OD.node_moments(net, model)
    obs, y = [], []
    for i, n in enumerate(pre):
        if n.leaf:
            r = list(taxa).index(n.name)
            for t in range(p):
                if tbl[t][r] is not None:
                    obs.append((i, t))
                    y.append(float(tbl[t][r]))
    idx = np.array([i * p + t for i, t in obs])
    S = cov[np.ix_(idx, idx)]
    X = np.zeros((len(obs), len(edges) * p))
    pos = {id(n): i for i, n in enumerate(pre)}
    for a, ed in enumerate(edges):
        tau = shift_transfer(net, model, pos[id(ed.child)])
        for r, (i, t) in enumerate(obs):
            X[r, a * p + t] = ed.gamma * tau[i]
    SiX = np.linalg.solve(S, X)
    H = X.T @ SiX
    shat = np.linalg.solve(H, SiX.T @ (np.array(y) - m0[idx])).reshape(len(edges), p)
    ll = OD.loglik(net, ShiftedModel(model, {ed.number: s for ed, s in zip(edges, shat)}), tbl, taxa)
    return shat, H, ll
