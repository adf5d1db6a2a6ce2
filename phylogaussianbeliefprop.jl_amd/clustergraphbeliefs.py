"""ClusterGraphBelief (src/clustergraphbeliefs.jl:26-109) backed by the device engine."""
import ctypes as C

import numpy as np

from . import _lib as L
from .beliefs import CanonicalBelief, MessageResidual, bclustertype, bsepsettype, scopeindex
from .beliefupdates import BPPosDefException


def _check(code, eng=None, lib=None):
    if code != L.PGBP_OK:
        lib = lib or L.load()
        msg = lib.pgbp_last_error(eng).decode() if lib else "?"
        raise L.PgbpError(code, msg)


class _BeliefList:
    """belief vector: CanonicalBelief objects whose h/J/g are views of the packed host mirror."""

    def __init__(self, owner):
        self._o = owner

    def __len__(self):
        return self._o.nbeliefs

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[k] for k in range(*i.indices(len(self)))]
        if i < 0:
            i += len(self)
        return self._o._belief_view(i)

    def __iter__(self):
        return (self[i] for i in range(len(self)))


class ClusterGraphBelief:
    """Device-resident ClusterGraphBelief.

    ClusterGraphBelief(beliefs, node2cluster, node2family, node2fixed, cluster2nodes)
    mirrors src/clustergraphbeliefs.jl:89-109: clusters first, sepsets last; builds cdict,
    sdict, the message residuals and the factors (copies of the initial cluster beliefs),
    precomputes scopeindex(sepset, cluster) for both ends of every sepset, and uploads.
    `ClusterGraphBelief.from_arrays` is the bulk constructor for large synthetic graphs."""

    def __init__(self, beliefs, node2cluster=None, node2family=None, node2fixed=None, cluster2nodes=None,
                 device=0):
        types = [b.type for b in beliefs]
        nc = types.index(bsepsettype) if bsepsettype in types else len(beliefs)
        if not all(t == bclustertype for t in types[:nc]):
            raise ValueError("clusters are not consecutive")
        if not all(t == bsepsettype for t in types[nc:]):
            raise ValueError("sepsets are not consecutive")
        cdict = {beliefs[j].metadata: j for j in range(nc)}
        dims = np.array([b.dimension for b in beliefs], dtype=np.int32)
        sepcl, off, idx = [], [0], []
        for j in range(nc, len(beliefs)):
            l1, l2 = beliefs[j].metadata
            a, b = cdict[l1], cdict[l2]
            sepcl += [a, b]
            for c in (a, b):
                ind = scopeindex(beliefs[j], beliefs[c])
                idx.append(ind)
                off.append(off[-1] + len(ind))
        idx = np.concatenate(idx) if idx else np.zeros(0, np.int32)
        self._init_common(dims, np.array(sepcl, np.int32), np.array(off, np.int64), idx, 1, device)
        self._objs = list(beliefs)
        self.cdict = cdict
        self.sdict = {frozenset(beliefs[j].metadata): j for j in range(nc, len(beliefs))}
        self.node2cluster, self.node2family = node2cluster, node2family
        self.node2fixed, self.cluster2nodes = node2fixed, cluster2nodes
        # copy h,J,g into the packed mirror and re-bind the objects' arrays to views of it
        for i, b in enumerate(self._objs):
            J, h, g = self._views(0, i)
            J[...] = b.J
            h[...] = b.h
            g[...] = b.g
            b.J, b.h, b.g = J, h, g
            b._owner, b._index = self, i
        self._upload(snapshot_factors=True)

    @classmethod
    def from_arrays(cls, dims, sepset_clusters, scope_off, scope_idx, packed, n_sites=1, device=0,
                    labels=None, engine=None):
        """Bulk constructor: description arrays of include/pgbp.h + packed (J,h,g) beliefs
        [n_sites, packed_size]; the cluster part is snapshot as the factors.  packed=None: nothing is uploaded and no
        host mirror is kept (large site batches whose factors are assigned on the device)."""
        self = cls.__new__(cls)
        self._init_common(np.asarray(dims, np.int32), np.asarray(sepset_clusters, np.int32).reshape(-1),
                          np.asarray(scope_off, np.int64), np.asarray(scope_idx, np.int32), n_sites, device, engine=engine)
        self._objs = None
        self._labels = labels
        self.cdict = self.sdict = None
        if packed is not None:   # None: all beliefs start as the constant 1 on the device (a device factor fill follows);
            self._packed[...] = np.asarray(packed, dtype=np.float64).reshape(self._packed.shape)   # no host mirror until a pull
            self._upload(snapshot_factors=True)
        return self

    # ------------------------------------------------------------------ internals
    def _init_common(self, dims, sepcl, scope_off, scope_idx, n_sites, device, engine=None):
        """engine: an engine created elsewhere for the same description (PatternGroup: pgbp_patterns_engine); it is
        borrowed, not destroyed with this object."""
        self._lib = L.load()
        self._eng = None
        self._borrowed = engine is not None
        self.n_sites = int(n_sites)
        self._dims = dims
        self.nsepsets = (len(scope_off) - 1) // 2
        self.nclusters = len(dims) - self.nsepsets
        self.nbeliefs = len(dims)
        self._sepcl = sepcl.reshape(-1, 2) if sepcl.size else np.zeros((0, 2), np.int32)
        self._scope_off, self._scope_idx = scope_off, scope_idx
        desc, self._keep = L.make_desc(dims, sepcl, scope_off, scope_idx, n_sites, device)
        eng = C.c_void_p()
        if engine is not None:
            eng = engine if isinstance(engine, C.c_void_p) else C.c_void_p(engine)
        else:
            code = self._lib.pgbp_create(C.byref(desc), C.byref(eng))
            if code != L.PGBP_OK:
                raise L.PgbpError(code, self._lib.pgbp_last_error(None).decode())
        self._eng = eng
        m = dims.astype(np.int64)
        self._poff = np.concatenate([[0], np.cumsum(m * m + m + 1)])
        s = np.repeat(dims[self.nclusters:].astype(np.int64), 2)
        self._roff = np.concatenate([[0], np.cumsum(s * s + s)])
        assert self._poff[-1] == self._lib.pgbp_packed_size(eng)
        assert self._roff[-1] == self._lib.pgbp_residual_size(eng)
        self._packed_arr = None   # host mirror [n_sites, packed_size], allocated at first use
        self._res = None
        self._flg = None
        self._kl = None
        self._klflg = None
        # LAZY write-back (one site): after a device call the mirror is only marked stale; a belief's record is fetched at
        # its first read (pgbp_get_belief), a residual's at its first read (pgbp_get_residual), the flag vectors on demand.
        # _stale: None = the mirror is current, else one bool per belief; _res_have: residual records fetched since the
        # last device call.  Engines with several sites keep the eager pull.
        self._stale = None
        self._n_single = 0
        self._res_have = None
        self.lazy = True
        self._schedule = None
        self.site = 0  # which site the belief views / residual views show
        self.belief = _BeliefList(self)
        self.messageresidual = _ResidualDict(self)
        self.last_results = None

    @property
    def _packed_raw(self):
        if self._packed_arr is None:
            self._packed_arr = np.zeros((self.n_sites, int(self._poff[-1])))
        return self._packed_arr

    @property
    def _packed(self):
        """the host mirror as a whole: made current first (what is still stale is fetched in one transfer)"""
        self._refresh_all()
        return self._packed_raw

    def _invalidate(self):
        """the device state changed: drop the host copies.  One site: lazily (nothing moves until something is read);
        several sites: the eager pull."""
        if self.n_sites == 1 and self.lazy:
            self._stale = np.ones(self.nbeliefs, dtype=bool)
            self._n_single = 0
            self._res = self._flg = self._kl = self._klflg = None
            self._res_have = None
        else:
            self.pull()

    def _refresh(self, i):
        if self._stale is None or not self._stale[i]:
            return
        self._n_single += 1
        if self._n_single > 64:   # a caller walking over the beliefs: one transfer of what is left beats thousands of small ones
            self._refresh_all()
            return
        n = int(self._poff[i + 1] - self._poff[i])
        rec = np.zeros(max(1, n))
        _check(self._lib.pgbp_get_belief(self._eng, 0, int(i), L.f64p(rec)), self._eng)
        self._packed_raw[0, self._poff[i]: self._poff[i + 1]] = rec[:n]
        self._stale[i] = False

    def _refresh_all(self):
        if self._stale is None:
            return
        idx = np.nonzero(self._stale)[0].astype(np.int32)
        if len(idx) == self.nbeliefs:
            _check(self._lib.pgbp_get_beliefs(self._eng, L.f64p(self._packed_raw)), self._eng)
        elif len(idx):
            # the stale records only, gathered on the device into one buffer (records edited on the host stay as they are)
            n = int(self._lib.pgbp_packed_beliefs_size(self._eng, len(idx), L.i32p(idx)))
            buf = np.zeros(max(1, n))
            _check(self._lib.pgbp_pack_beliefs(self._eng, 0, len(idx), L.i32p(idx), L.f64p(buf)), self._eng)
            at = 0
            for i in idx:
                m = int(self._poff[i + 1] - self._poff[i])
                self._packed_raw[0, self._poff[i]: self._poff[i + 1]] = buf[at: at + m]
                at += m
        self._stale = None

    def __del__(self):
        try:
            if getattr(self, "_eng", None):
                if not getattr(self, "_borrowed", False):
                    self._lib.pgbp_destroy(self._eng)
                self._eng = None
        except Exception:
            pass

    def _views(self, site, i):
        m = int(self._dims[i])
        self._refresh(i)
        rec = self._packed_raw[site, self._poff[i]: self._poff[i + 1]]
        return rec[: m * m].reshape(m, m, order="F"), rec[m * m: m * m + m], rec[m * m + m:]

    def _belief_view(self, i):
        if self._objs is not None and self.site == 0:
            return self._objs[i]
        J, h, g = self._views(self.site, i)
        site_is_lazy = self.n_sites == 1
        b = CanonicalBelief.__new__(CanonicalBelief)
        b.nodelabel, b.ntraits, b.inscope = None, None, None
        b.J, b.h, b.g, b.mu = J, h, g, np.zeros(len(h))
        if site_is_lazy:
            b._owner, b._index = self, i
        b.type = bclustertype if i < self.nclusters else bsepsettype
        b.metadata = self._labels[i] if getattr(self, "_labels", None) is not None else i
        return b

    def _upload(self, snapshot_factors=False):
        # (self._packed: whatever of the mirror is stale is fetched first, so an upload never writes old values back)
        _check(self._lib.pgbp_set_beliefs(self._eng, L.f64p(self._packed), int(snapshot_factors)), self._eng)

    def push(self):
        """host mirror -> device (after editing belief arrays on the host)."""
        self._upload(False)

    def pull(self):
        """device -> host mirror, everything at once: beliefs, residuals, flags (the eager write-back)."""
        self._stale = None
        _check(self._lib.pgbp_get_beliefs(self._eng, L.f64p(self._packed_raw)), self._eng)
        self._res_have = None
        nm = 2 * self.nsepsets
        self._res = np.zeros((self.n_sites, max(1, int(self._roff[-1]))))
        self._flg = np.zeros((self.n_sites, max(1, nm)), dtype=np.int32)
        self._kl = np.zeros((self.n_sites, max(1, nm)))
        self._klflg = np.zeros((self.n_sites, max(1, nm)), dtype=np.int32)
        _check(self._lib.pgbp_get_residuals(self._eng, L.f64p(self._res), L.i32p(self._flg), L.f64p(self._kl),
                                            L.i32p(self._klflg)), self._eng)

    def _fetch_words(self):
        """flags, kldiv, iscalibrated_kl of every message (no residual record moves)"""
        nm = 2 * self.nsepsets
        self._flg = np.zeros((self.n_sites, max(1, nm)), dtype=np.int32)
        self._kl = np.zeros((self.n_sites, max(1, nm)))
        self._klflg = np.zeros((self.n_sites, max(1, nm)), dtype=np.int32)
        _check(self._lib.pgbp_get_residuals(self._eng, None, L.i32p(self._flg), L.f64p(self._kl), L.i32p(self._klflg)), self._eng)

    def _residual_record(self, d):
        if self._res is None and not (self.n_sites == 1 and self.lazy):
            self.pull()
        if self._res is None:   # lazy: one record at a time
            self._res = np.zeros((1, max(1, int(self._roff[-1]))))
            self._res_have = np.zeros(2 * self.nsepsets, dtype=bool)
        if self._res_have is not None and not self._res_have[d] and int(self._res_have.sum()) >= 64:
            # a caller walking over the residuals: the rest in one transfer
            _check(self._lib.pgbp_get_residuals(self._eng, L.f64p(self._res), None, None, None), self._eng)
            self._res_have = None
        if self._res_have is not None and not self._res_have[d]:
            n = int(self._roff[d + 1] - self._roff[d])
            rec = np.zeros(max(1, n))
            _check(self._lib.pgbp_get_residual(self._eng, 0, int(d), L.f64p(rec), None, None, None), self._eng)
            self._res[0, self._roff[d]: self._roff[d + 1]] = rec[:n]
            self._res_have[d] = True
        return self._res[self.site, self._roff[d]: self._roff[d + 1]]

    def _residual_words(self, d):
        """(iscalibrated_resid, kldiv, iscalibrated_kl) of message d"""
        if self._flg is None:
            self._fetch_words()
        return self._flg[self.site][d], self._kl[self.site][d], self._klflg[self.site][d]

    def _flags(self):
        if self._flg is None:
            self._fetch_words()
        return self._flg[self.site]

    def _kldiv(self):
        if self._kl is None:
            self._fetch_words()
        return self._kl[self.site]

    def _klflags(self):
        if getattr(self, "_klflg", None) is None:
            self._fetch_words()
        return self._klflg[self.site]

    def residual_kldiv_(self, cluster_to, sepset, cluster_from, atol=1e-5):
        """residual_kldiv!(messageresidual[(to, from)], sepset) (src/beliefs.jl:1060-1075) on belief indices:
        updates kldiv / iscalibrated_kl of that residual on the device and returns the flag."""
        out = np.zeros(self.n_sites, dtype=np.int32)
        o = self._opts(atol=atol)
        _check(self._lib.pgbp_residual_kldiv(self._eng, int(cluster_to), int(sepset), int(cluster_from), C.byref(o),
                                             L.i32p(out)), self._eng)
        self._flg = self._kl = self._klflg = None   # (the beliefs and the residual records are untouched)
        if int(self._dims[sepset]) == 0:
            return True
        return bool(out[self.site])

    def _msg_id(self, receiver, sender):
        for k in range(self.nsepsets):
            a, b = self._sepcl[k]
            if a == receiver and b == sender:
                return 2 * k
            if b == receiver and a == sender:
                return 2 * k + 1
        raise KeyError((receiver, sender))

    def _opts(self, auto=False, update_residualnorm=True, update_residualkldiv=False, atol=1e-5):
        return L.Opts(int(auto), int(update_residualnorm), int(update_residualkldiv), 0, float(atol))

    def _integrate_index_1based(self, sender, sepset_k, side):
        o0, o1 = self._scope_off[2 * sepset_k + side], self._scope_off[2 * sepset_k + side + 1]
        keep = set(self._scope_idx[o0:o1].tolist())
        return [i + 1 for i in range(int(self._dims[sender])) if i not in keep]

    def _exception_for(self, sender, sepset_k, info):
        """"belief $metadata, integrating $(integrate_index)" (src/beliefupdates.jl:71)."""
        side = 0 if self._sepcl[sepset_k][0] == sender else 1
        meta = self._belief_label(sender)
        idx = self._integrate_index_1based(sender, sepset_k, side)
        return BPPosDefException(f"belief {meta}, integrating {idx}", info)

    def _belief_label(self, i):
        if self._objs is not None:
            return self._objs[i].metadata
        if getattr(self, "_labels", None) is not None:
            return self._labels[i]
        return i

    def _propagate(self, cluster_to, sepset, cluster_from, sync=True):
        info = np.zeros(self.n_sites, dtype=np.int32)
        o = self._opts()
        _check(self._lib.pgbp_propagate(self._eng, int(cluster_to), int(sepset), int(cluster_from), C.byref(o),
                                        L.i32p(info)), self._eng)
        if sync:
            self._invalidate()
        if info[self.site] != 0:
            return self._exception_for(cluster_from, sepset - self.nclusters, int(info[self.site]))
        return None

    # ------------------------------------------------------------------ reference API
    def clusterindex(self, label):
        return self.cdict[label]

    def sepsetindex(self, l1, l2):
        return self.sdict[frozenset((l1, l2))]

    def set_schedule(self, schedule):
        """schedule: list of spanning trees (pa_lab, ch_lab, pa_j, ch_j) as spanningtree_clusterlist
        returns them (src/clustergraph.jl:885-894), or just (pa_j, ch_j); 0-based cluster indices."""
        trees = [(np.asarray(t[-2], np.int32), np.asarray(t[-1], np.int32)) for t in schedule]
        off = np.zeros(len(trees) + 1, dtype=np.int32)
        for i, (pa, _) in enumerate(trees):
            off[i + 1] = off[i] + len(pa)
        pa = np.concatenate([t[0] for t in trees]) if trees else np.zeros(0, np.int32)
        ch = np.concatenate([t[1] for t in trees]) if trees else np.zeros(0, np.int32)
        pa = np.ascontiguousarray(pa if pa.size else np.zeros(1, np.int32))
        ch = np.ascontiguousarray(ch if ch.size else np.zeros(1, np.int32))
        _check(self._lib.pgbp_set_schedule(self._eng, len(trees), L.i32p(off), L.i32p(pa), L.i32p(ch)), self._eng)
        self._schedule = [(t[0].copy(), t[1].copy()) for t in trees]

    def _ensure_schedule(self, schedule):
        trees = [(np.asarray(t[-2], np.int32), np.asarray(t[-1], np.int32)) for t in schedule]
        same = self._schedule is not None and len(trees) == len(self._schedule) and all(
            np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(trees, self._schedule))
        if not same:
            self.set_schedule(schedule)

    def init_beliefs_reset_fromfactors_(self, sync=True):
        """init_beliefs_reset_fromfactors! (src/clustergraphbeliefs.jl:126-139)."""
        _check(self._lib.pgbp_reset_from_factors(self._eng), self._eng)
        if sync:
            self._invalidate()

    def init_factors_frombeliefs_(self):
        """init_factors_frombeliefs! (src/beliefs.jl:746-761) on the device state."""
        _check(self._lib.pgbp_init_factors_frombeliefs(self._eng), self._eng)

    def init_messagecalibrationflags_reset_(self, reset_kl=True):
        """init_messagecalibrationflags_reset! (src/clustergraphbeliefs.jl:146-150)."""
        _check(self._lib.pgbp_reset_flags(self._eng, int(reset_kl)), self._eng)
        self._flg = self._kl = self._klflg = None

    def iscalibrated_residnorm(self):
        """iscalibrated_residnorm(beliefs) (src/clustergraphbeliefs.jl:168-169)."""
        self._fetch_words()   # (the flag vectors alone: no belief, no residual record moves)
        return bool(np.all(self._flg[self.site][: 2 * self.nsepsets] != 0))

    def integratebelief_(self, j, all_sites=False):
        """integratebelief!(obj, beliefindex) (src/clustergraphbeliefs.jl:194): (mu, norm)."""
        m = int(self._dims[j])
        mu = np.zeros((self.n_sites, max(1, m)))
        norm = np.zeros(self.n_sites)
        info = np.zeros(self.n_sites, dtype=np.int32)
        _check(self._lib.pgbp_integrate(self._eng, int(j), L.f64p(mu), L.f64p(norm), L.i32p(info)), self._eng)
        mu = mu.reshape(-1)[: self.n_sites * m].reshape(self.n_sites, m)
        if all_sites:
            return mu, norm, info
        if info[self.site] != 0:
            raise np.linalg.LinAlgError(
                f"PosDefException: matrix is not positive definite; Cholesky factorization failed (info={info[self.site]}).")
        if self._objs is not None and self.site == 0:
            self._objs[j].mu = mu[0].copy()
        return mu[self.site].copy(), float(norm[self.site])

    def moments_(self, beliefs=None, cov=True, all_sites=False):
        """Posterior moments of many beliefs in ONE device call (pgbp_moments): per listed belief (beliefs=None: every
        cluster) the tuple (mu, Sigma, norm) with Sigma = J^-1 (None when cov is false); mu and norm are
        integratebelief!'s (src/beliefupdates.jl:168-200), bit for bit those of integratebelief_.  all_sites: the arrays
        gain a leading site axis and a fourth element, info [n_sites] (0, or PosDefException.info: that site's entries
        are NaN); otherwise the current site's values, and a belief of the current site that is not positive definite
        raises integratebelief_'s LinAlgError."""
        if beliefs is None:
            lst = np.arange(self.nclusters, dtype=np.int32)
            ptr, n = None, 0
        else:
            lst = np.ascontiguousarray(beliefs, dtype=np.int32).reshape(-1)
            keep = lst if lst.size else np.zeros(1, dtype=np.int32)
            ptr, n = L.i32p(keep), int(lst.size)
        per = int(self._lib.pgbp_moments_size(self._eng, n, ptr, int(bool(cov))))
        if per < 0:
            # (the call itself reports which index is bad / which belief is too large)
            _check(self._lib.pgbp_moments(self._eng, n, ptr, 0, 0, int(bool(cov)), None, None), self._eng)
            raise L.PgbpError(L.ERR_INVALID, "pgbp_moments_size failed")
        s0, s1 = (0, self.n_sites) if all_sites else (self.site, self.site + 1)
        out = np.zeros((s1 - s0, max(1, per)))
        info = np.zeros((s1 - s0, max(1, lst.size)), dtype=np.int32)
        _check(self._lib.pgbp_moments(self._eng, n, ptr, s0, s1, int(bool(cov)), L.f64p(out), L.i32p(info)), self._eng)
        res, at = [], 0
        for i, b in enumerate(lst):
            m = int(self._dims[b])
            Sig = None
            if cov:
                # (column-major records; the site count spelled out: -1 cannot be inferred for a belief without variables)
                Sig = out[:, at: at + m * m].reshape(out.shape[0], m, m).transpose(0, 2, 1)
                at += m * m
            mu = out[:, at: at + m]
            norm = out[:, at + m]
            at += m + 1
            if all_sites:
                res.append((mu.copy(), None if Sig is None else Sig.copy(), norm.copy(), info[:, i].copy()))
                continue
            if info[0, i] != 0:
                raise np.linalg.LinAlgError(
                    f"PosDefException: matrix is not positive definite; Cholesky factorization failed (info={info[0, i]}).")
            res.append((mu[0].copy(), None if Sig is None else Sig[0].copy(), float(norm[0])))
        return res

    def sample_posterior_(self, n_draws=1, z=None, rng=None, schedule_tree=0, all_sites=False):
        """Joint posterior draws of every cluster variable in ONE device call (pgbp_sample_posterior): a preorder sweep of
        schedule tree `schedule_tree` (an index into the schedule that was set, as pgbp_traverse's `tree`) that conditions
        each cluster on the sepset to its parent.  A draw from the joint posterior only if the beliefs are calibrated
        (postorder and preorder) on a clique tree; the call does not verify that.
        z: standard normals [n_draws, n_sites or 1, size] (size = the sum of the cluster dimensions); None: drawn with
        numpy.random.default_rng(rng).  z = 0 gives the joint posterior mean.
        Returns (x, info, views): x [n_draws, n_sites or 1, size] (all_sites: every site, otherwise the current one),
        info [n_sites or 1] (0, or the 1-based index of the first cluster in preorder whose conditional precision is not
        positive definite: that site's draws are NaN) and views[i] = x[:, :, cluster i's variables]."""
        size = int(self._lib.pgbp_sample_size(self._eng))
        s0, s1 = (0, self.n_sites) if all_sites else (self.site, self.site + 1)
        n_draws = int(n_draws)
        shape = (max(n_draws, 0), s1 - s0, size)
        if z is None:
            z = np.random.default_rng(rng).standard_normal(shape)
        z = np.ascontiguousarray(z, dtype=np.float64)
        if z.shape != shape:
            raise ValueError(f"z has shape {z.shape}, expected {shape}")
        x = np.zeros(shape)
        info = np.zeros(s1 - s0, dtype=np.int32)
        keep = z if z.size else np.zeros(1)
        out = x if x.size else np.zeros(1)
        _check(self._lib.pgbp_sample_posterior(self._eng, int(schedule_tree), s0, s1, n_draws, L.f64p(keep), L.f64p(out),
                                               L.i32p(info)), self._eng)
        off = np.concatenate([[0], np.cumsum(self._dims[: self.nclusters].astype(np.int64))])
        return x, info, [x[:, :, off[i]: off[i + 1]] for i in range(self.nclusters)]

    def node_samples(self, draws, site=0):
        """The draws of sample_posterior_ by node, for an object built from labelled beliefs: {node label: [n_draws, p]},
        the traits of a node that are out of scope NaN, the values taken from the first cluster that holds the node.
        draws: x [n_draws, sites, size]; site: which of its site columns."""
        if self._objs is None:
            raise ValueError("node_samples needs labelled beliefs (an object built from CanonicalBelief objects)")
        draws = np.asarray(draws)
        out, at = {}, 0
        for b in self._objs[: self.nclusters]:
            insc = np.asarray(b.inscope, dtype=bool)
            for k, lab in enumerate(b.nodelabel):
                n = int(insc[:, k].sum())
                if lab not in out:
                    v = np.full((draws.shape[0], insc.shape[0]), np.nan)
                    v[:, insc[:, k]] = draws[:, site, at: at + n]
                    out[lab] = v
                at += n
        return out

    def posterior_cov_(self, c, schedule_tree=0, all_sites=False, want_w=True, want_k=True):
        """Exact posterior covariances of linear functionals of the cluster variables in ONE device call
        (pgbp_posterior_cov): the adjoint of sample_posterior_'s sweep, x = m + A z at one site.
        c: [n_cols, size] (or [size]), a weight per entry of sample_posterior_'s layout, shared by the sites.
        Returns (w, k, info): w [n_cols, n_sites or 1, size] = A'c, so that w_a . w_b = Cov(c_a'x, c_b'x | data), +0.0 at the
        entries the sampler conditions on; k [n_cols, n_sites or 1, size] = A w = Cov(x, c'x | data), the covariance of every
        entry with the functional; info as sample_posterior_'s (a site whose info is not 0 is NaN).  want_w / want_k false:
        that array is None (without k no forward pass is run).  Exact only if the beliefs are calibrated on a clique tree;
        the call does not verify that."""
        size = int(self._lib.pgbp_sample_size(self._eng))
        s0, s1 = (0, self.n_sites) if all_sites else (self.site, self.site + 1)
        c = np.ascontiguousarray(np.atleast_2d(np.asarray(c, dtype=np.float64)))
        if c.ndim != 2 or c.shape[1] != size:
            raise ValueError(f"c has shape {c.shape}, expected (n_cols, {size})")
        shape = (c.shape[0], s1 - s0, size)
        w = np.zeros(shape) if want_w else None
        k = np.zeros(shape) if want_k else None
        info = np.zeros(s1 - s0, dtype=np.int32)
        ptr = lambda a: None if a is None else L.f64p(a if a.size else np.zeros(1))
        _check(self._lib.pgbp_posterior_cov(self._eng, int(schedule_tree), s0, s1, int(c.shape[0]),
                                            L.f64p(c if c.size else np.zeros(1)), ptr(w), ptr(k), L.i32p(info)), self._eng)
        return w, k, info

    def _node_entries(self, who):
        """{node label: (cluster, positions in the cluster [p], entries of sample_posterior_'s layout [p])} from the first
        cluster that holds the node (node_samples' rule); -1 where the trait is out of scope."""
        if self._objs is None:
            raise ValueError(f"{who} needs labelled beliefs (an object built from CanonicalBelief objects)")
        out, at = {}, 0
        for ci, b in enumerate(self._objs[: self.nclusters]):
            insc = np.asarray(b.inscope, dtype=bool)
            inside = 0
            for k, lab in enumerate(b.nodelabel):
                n = int(insc[:, k].sum())
                if lab not in out:
                    pos = np.full(insc.shape[0], -1, dtype=np.int64)
                    pos[insc[:, k]] = inside + np.arange(n)
                    out[lab] = (ci, pos, np.where(pos >= 0, at - inside + pos, -1))
                at += n
                inside += n
        return out

    def sample_index(self, node, trait):
        """The entry of sample_posterior_'s layout (a column of x, an index into a row of c) of trait `trait` of the node
        labelled `node`, in the first cluster that holds the node; -1 when that trait is out of scope there."""
        ent = self._node_entries("sample_index")
        if node not in ent:
            raise ValueError(f"no cluster holds node {node!r}")
        return int(ent[node][2][int(trait)])

    def _node_means(self, ent, nodes):
        """posterior means [len(nodes), p] from moments_ (NaN out of scope)"""
        clusters = sorted({ent[v][0] for v in nodes})
        mom = dict(zip(clusters, self.moments_(clusters, cov=False)))
        out = np.full((len(nodes), len(ent[nodes[0]][1]) if nodes else 0), np.nan)
        for i, v in enumerate(nodes):
            ci, pos, _ = ent[v]
            out[i, pos >= 0] = mom[ci][0][pos[pos >= 0]]
        return out

    def node_cov(self, nodes_a, nodes_b=None, schedule_tree=0):
        """Posterior covariance blocks between nodes that need not share a cluster: [len(a), len(b), p, p], entry
        [i, j, s, t] = Cov(trait s of a_i, trait t of b_j | data) at the current site; nodes_b=None: nodes_a among
        themselves.  One column of posterior_cov_ per in-scope (node of b, trait); traits out of scope are NaN."""
        ent = self._node_entries("node_cov")
        nodes_a = list(nodes_a)
        nodes_b = nodes_a if nodes_b is None else list(nodes_b)
        for v in nodes_a + nodes_b:
            if v not in ent:
                raise ValueError(f"no cluster holds node {v!r}")
        size = int(self._lib.pgbp_sample_size(self._eng))
        cols = [(j, t, int(e)) for j, v in enumerate(nodes_b) for t, e in enumerate(ent[v][2]) if e >= 0]
        p = len(next(iter(ent.values()))[1]) if ent else 0
        out = np.full((len(nodes_a), len(nodes_b), p, p), np.nan)
        if not cols or not nodes_a:
            return out
        c = np.zeros((len(cols), size))
        c[np.arange(len(cols)), [e for _, _, e in cols]] = 1.0
        _, k, info = self.posterior_cov_(c, schedule_tree, want_w=False)
        if info[0] != 0:
            raise np.linalg.LinAlgError(f"PosDefException: the conditional precision of cluster {info[0]} is not positive definite.")
        for i, v in enumerate(nodes_a):
            ea = ent[v][2]
            for q, (j, t, _) in enumerate(cols):
                out[i, j, ea >= 0, t] = k[q, 0, ea[ea >= 0]]
        return out

    def nodes_joint_posterior(self, nodes, schedule_tree=0):
        """The joint posterior of several nodes, wherever they sit in the clique tree (an out-of-clique query):
        (mean [n, p], cov [n p, n p]), node-major; the mean from moments_, the covariance from node_cov."""
        nodes = list(nodes)
        cov = self.node_cov(nodes, None, schedule_tree)
        n, p = cov.shape[0], cov.shape[2]
        return self._node_means(self._node_entries("nodes_joint_posterior"), nodes), cov.transpose(0, 2, 1, 3).reshape(n * p, n * p)

    def functional_moments(self, weights, schedule_tree=0):
        """Posterior mean [q] and covariance [q, q] of the q linear functionals sum_v W_v x_v; weights: {node label: W_v [q, p]}.
        The covariance is w w' of posterior_cov_ (no forward pass).  A non-zero weight on a trait out of scope is refused."""
        ent = self._node_entries("functional_moments")
        nodes = list(weights)
        size = int(self._lib.pgbp_sample_size(self._eng))
        W = [np.atleast_2d(np.asarray(weights[v], dtype=np.float64)) for v in nodes]
        q = W[0].shape[0] if W else 0
        c = np.zeros((q, size))
        for v, Wv in zip(nodes, W):
            if v not in ent:
                raise ValueError(f"no cluster holds node {v!r}")
            e = ent[v][2]
            if Wv.shape != (q, len(e)):
                raise ValueError(f"the weights of node {v!r} have shape {Wv.shape}, expected {(q, len(e))}")
            if np.any(Wv[:, e < 0] != 0.0):
                raise ValueError(f"node {v!r}: weight on a trait that is out of scope")
            c[:, e[e >= 0]] += Wv[:, e >= 0]
        if q == 0:
            return np.zeros(0), np.zeros((0, 0))
        w, _, info = self.posterior_cov_(c, schedule_tree, want_k=False)
        if info[0] != 0:
            raise np.linalg.LinAlgError(f"PosDefException: the conditional precision of cluster {info[0]} is not positive definite.")
        mu = np.nan_to_num(self._node_means(ent, nodes))
        mean = sum((Wv @ m for Wv, m in zip(W, mu)), np.zeros(q))
        return mean, w[:, 0] @ w[:, 0].T

    def default_sepset1(self):
        """default_sepset1 (src/clustergraphbeliefs.jl:197-202)."""
        for j in range(self.nclusters, self.nbeliefs):
            if len(self._objs[j].nodelabel) == 1:
                return j
        raise ValueError("no sepset with a single node")

    # ------------------------------------------------------------------ scores (src/score.jl)
    def free_energy(self, all_sites=False):
        """free_energy(beliefs) (src/score.jl:162-182): (average energy, approximate entropy, free energy)."""
        out = np.zeros((self.n_sites, 3))
        info = np.zeros(self.n_sites, dtype=np.int32)
        _check(self._lib.pgbp_free_energy(self._eng, L.f64p(out), L.i32p(info)), self._eng)
        if all_sites:
            return out, info
        if info[self.site]:
            raise np.linalg.LinAlgError(f"PosDefException: belief {info[self.site] - 1} is not positive definite")
        return tuple(float(x) for x in out[self.site])

    def factored_energy(self):
        """factored_energy(beliefs) (src/score.jl:151-154): third value = -free energy."""
        a, e, f = self.free_energy()
        return (a, e, -f)

    # ------------------------------------------------------------------ device factor assignment
    def bm_tree_setup(self, kind, length, data_row, data):
        """Static part of assignfactors! for a homogeneous BM on a tree (include/pgbp.h: pgbp_bm_tree);
        data: [n_sites, n_rows, p] (or [n_rows, p] for one site) tip data indexed by data_row."""
        data = np.ascontiguousarray(np.asarray(data, np.float64))
        if data.ndim == 2:
            data = data[None]
        assert data.shape[0] == self.n_sites
        self._bm = dict(kind=np.ascontiguousarray(kind, np.int32), length=np.ascontiguousarray(length, np.float64),
                        row=np.ascontiguousarray(data_row, np.int32), data=data)
        t = L.BmTree(int(data.shape[2]), int(data.shape[1]), L.i32p(self._bm["kind"]), L.f64p(self._bm["length"]),
                     L.i32p(self._bm["row"]), L.f64p(data))
        _check(self._lib.pgbp_bm_tree_setup(self._eng, C.byref(t)), self._eng)
        self._bm_p = int(data.shape[2])

    def assignfactors_bm_(self, R, mu, sync=False):
        """assignfactors!(beliefs, MvFullBrownianMotion(R, mu), ...) (src/beliefs.jl:786-861) on the device:
        only R^-1, log det R and mu cross the bus.  R: [p, p] or [n_sites, p, p]; mu: [p] or [n_sites, p]."""
        R = np.asarray(R, np.float64)
        mu = np.asarray(mu, np.float64)
        per_site = R.ndim == 3
        Rs = R if per_site else R[None]
        Rinv = np.ascontiguousarray(np.stack([np.linalg.inv((r + r.T) / 2) for r in Rs]))
        Rinv = np.ascontiguousarray((Rinv + np.transpose(Rinv, (0, 2, 1))) / 2)
        logdet = np.ascontiguousarray([np.linalg.slogdet(r)[1] for r in Rs], np.float64)
        mus = np.ascontiguousarray(mu if mu.ndim == 2 else np.broadcast_to(mu, (len(Rs), self._bm_p)).copy())
        _check(self._lib.pgbp_bm_tree_assignfactors(self._eng, L.f64p(Rinv), L.f64p(logdet), L.f64p(mus),
                                                    int(per_site)), self._eng)
        if sync:
            self._invalidate()

    def lg_setup(self, fam, data):
        """Static part of assignfactors! for any linear-Gaussian model (include/pgbp.h: pgbp_lg_families).
        fam: the dictionary factors.lg_families(...) returns; data: [n_sites, n_rows, p] (or [n_rows, p]) tip data."""
        data = np.ascontiguousarray(np.asarray(data, np.float64))
        if data.ndim == 2:
            data = data[None]
        assert data.shape[0] == self.n_sites and data.shape[2] == fam["p"]
        if fam.get("child_mask") is not None:
            assert fam["parent_mask"].size == len(fam["cluster"]) * max(1, int(fam["max_parents"]))
        k = {n: np.ascontiguousarray(fam[n], np.int32) for n in ("cluster", "n_parents", "child_pos", "data_row",
                                                                 "parent_pos", "color")}
        k.update({n: np.ascontiguousarray(fam[n], np.float64) for n in ("length", "gamma")})
        k["data"] = data
        for n in ("child_mask", "parent_mask"):
            k[n] = np.ascontiguousarray(fam[n], np.uint64) if fam.get(n) is not None else None
        self._lg = k  # keep alive
        nf = len(k["cluster"])
        K = max(1, int(fam["max_parents"]))
        for n in ("parent_pos", "color", "length", "gamma"):
            assert k[n].size == nf * K, n
        t = L.LgFamilies(int(fam["p"]), nf, K, int(fam["n_rates"]), int(data.shape[1]), L.i32p(k["cluster"]),
                         L.i32p(k["n_parents"]), L.i32p(k["child_pos"]), L.i32p(k["data_row"]), L.i32p(k["parent_pos"]),
                         L.f64p(k["length"]), L.f64p(k["gamma"]), L.i32p(k["color"]), L.f64p(data),
                         k["child_mask"].ctypes.data_as(C.POINTER(C.c_uint64)) if k["child_mask"] is not None else None,
                         k["parent_mask"].ctypes.data_as(C.POINTER(C.c_uint64)) if k["parent_mask"] is not None else None)
        _check(self._lib.pgbp_lg_setup(self._eng, C.byref(t)), self._eng)
        self._lg_p, self._lg_nrates = int(fam["p"]), int(fam["n_rates"])
        if fam.get("parent_family") is not None:       # who the parents are (pgbp_lg_set_topology): simulate_lg needs it
            k["parent_family"] = np.ascontiguousarray(fam["parent_family"], np.int32).reshape(-1)
            assert k["parent_family"].size == nf * K, "parent_family"
            _check(self._lib.pgbp_lg_set_topology(self._eng, L.i32p(k["parent_family"])), self._eng)
        self._lg_shift_edges = np.zeros(0, np.int32)   # a new table clears the shifts (pgbp_lg_setup)
        self._lg_noise = None                          # ... and the tip noise
        self._lg_optima = None                         # ... and the painted optima
        self._lg_last = None                           # ... and has no parameters yet
        self._lg_data_nan = np.isnan(data[:, :, 0]) if int(fam["p"]) == 1 else None   # (set_site_missing_lg("nan"); no mask yet)
        self._lg_site_mask = None                      # ... and no per-site mask

    def assignfactors_lg_(self, R, mu, model="bm", alpha=None, theta=None, sync=False):
        """assignfactors!(beliefs, model, ...) (src/beliefs.jl:786-861) on the device for a Brownian motion
        (homogeneous / heterogeneous: R = the variance rate(s)) or an Ornstein-Uhlenbeck process (R = stationary
        variance), on the families given to lg_setup; only the model parameters cross the bus.
        R: [n_rates, p, p] or, per site, [n_sites, n_rates, p, p]; mu / theta: [p] or [n_sites, p]; alpha: scalar or
        [n_sites].  A random root's prior variance is one more entry of R (the root family's colour)."""
        p, nr = self._lg_p, self._lg_nrates
        R = np.asarray(R, np.float64)
        per_site = R.ndim == 4
        n = self.n_sites if per_site else 1
        R = np.ascontiguousarray(R.reshape(n, nr, p, p).transpose(0, 1, 3, 2))  # column-major blocks
        mu = np.ascontiguousarray(np.broadcast_to(np.asarray(mu, np.float64).reshape(-1, p), (n, p)))
        ou = model == "ou"
        al = np.ascontiguousarray(np.broadcast_to(np.asarray(alpha if ou else 0.0, np.float64).reshape(-1), (n,)))
        th = np.ascontiguousarray(np.broadcast_to(np.asarray(theta if ou else np.zeros(p), np.float64).reshape(-1, p), (n, p)))
        m = L.LgParams(L.LG_OU if ou else L.LG_BM, int(per_site), L.f64p(R), L.f64p(al) if ou else None,
                       L.f64p(th) if ou else None, L.f64p(mu))
        _check(self._lib.pgbp_lg_assignfactors(self._eng, C.byref(m)), self._eng)
        self._lg_last = (m, (R, mu, al, th))   # what loglik_and_shift_gradient_lg fills again (keeps the arrays alive)
        if sync:
            self._invalidate()

    def loglik_lg(self, reps=1):
        """The body of score(theta) (src/calibration.jl:195-221) on the device with the parameters of the last
        assignfactors_lg_: factor fill, postorder of schedule tree 0, root integrate.  Returns (loglik[n_sites], info)."""
        o = self._opts()
        _check(self._lib.pgbp_enqueue_loglik_lg(self._eng, int(reps), C.byref(o)), self._eng)
        norm = np.zeros(self.n_sites)
        info = np.zeros(self.n_sites, dtype=np.int32)
        _check(self._lib.pgbp_fetch_loglik(self._eng, L.f64p(norm), L.i32p(info)), self._eng)
        return norm, info

    def gradient_lg(self, all_sites=False):
        """pgbp_lg_gradient on the current beliefs: the gradient of the log-likelihood with respect to every parameter
        of the last assignfactors_lg_, by Fisher's identity -- one sweep over the node families.  EXACT ONLY when the
        beliefs are calibrated (postorder and preorder) on a clique tree under those parameters (not verified); on a
        loopy cluster graph, at a converged calibration, it is the gradient of the factored energy.
        Returns a dict: dR [n_rates, p, p] (symmetric; d loglik = sum_c tr(dR[c] dR_c)), dmu [p], dalpha (scalar) and
        dtheta [p] (zero for a Brownian motion), info; with a leading site axis when all_sites.  A site whose info is
        not 0 (1-based index of a cluster that is not positive definite) holds NaN; for the current site that raises.
        With tip noise set (set_tip_noise_lg) the dict also holds dsigma_e [p, p] (symmetric; d loglik = tr(dsigma_e
        dSigma_e)): pgbp_lg_gradient_noise.  With painted optima set (set_optima_lg) it also holds doptima [n_regimes, p],
        the derivative in each regime's optimum (0 for a regime no edge carries); dtheta is then the derivative in theta of
        the unpainted edges alone: pgbp_lg_gradient_optima."""
        p, nr = self._lg_p, self._lg_nrates
        s0, s1 = (0, self.n_sites) if all_sites else (self.site, self.site + 1)
        n = s1 - s0
        dR = np.zeros((n, nr, p, p))
        dmu = np.zeros((n, p))
        dalpha = np.zeros(n)
        dtheta = np.zeros((n, p))
        info = np.zeros(n, dtype=np.int32)
        noisy = self.tip_noise_count_lg() > 0
        nopt = self.optima_count_lg()
        if nopt > 0:   # painted optima: dtheta covers the unpainted edges, doptima [n_regimes, p] the painted ones
            dsig = np.zeros((n, p, p)) if noisy else None
            dopt = np.zeros((n, nopt, p))
            _check(self._lib.pgbp_lg_gradient_optima(self._eng, s0, s1, L.f64p(dR), L.f64p(dmu), L.f64p(dalpha),
                                                     L.f64p(dtheta), L.f64p(dsig) if noisy else None, L.f64p(dopt),
                                                     L.i32p(info)), self._eng)
        elif noisy:
            dsig = np.zeros((n, p, p))
            _check(self._lib.pgbp_lg_gradient_noise(self._eng, s0, s1, L.f64p(dR), L.f64p(dmu), L.f64p(dalpha),
                                                    L.f64p(dtheta), L.f64p(dsig), L.i32p(info)), self._eng)
        else:
            _check(self._lib.pgbp_lg_gradient(self._eng, s0, s1, L.f64p(dR), L.f64p(dmu), L.f64p(dalpha), L.f64p(dtheta),
                                              L.i32p(info)), self._eng)
        dR = dR.transpose(0, 1, 3, 2)   # (column-major blocks; symmetric)
        d = dict(dR=dR, dmu=dmu, dalpha=dalpha, dtheta=dtheta, info=info)
        if noisy:
            d["dsigma_e"] = dsig.transpose(0, 2, 1)
        if nopt > 0:
            d["doptima"] = dopt
        return d if all_sites else self._gradient_of_site(d, 0)

    @staticmethod
    def _gradient_of_site(d, s):
        if d["info"][s]:
            raise np.linalg.LinAlgError(f"PosDefException: belief {d['info'][s] - 1} is not positive definite")
        out = dict(dR=d["dR"][s].copy(), dmu=d["dmu"][s].copy(), dalpha=float(d["dalpha"][s]), dtheta=d["dtheta"][s].copy(),
                   info=0)
        if "dsigma_e" in d:
            out["dsigma_e"] = d["dsigma_e"][s].copy()
        if "doptima" in d:
            out["doptima"] = d["doptima"][s].copy()
        return out

    def loglik_and_gradient_lg(self, schedule_tree, all_sites=False):
        """Log-likelihood and its exact gradient under the parameters of the last assignfactors_lg_ on a clique tree:
        beliefs reset from the factors that call filled -> one calibrate (postorder + preorder of `schedule_tree`) ->
        integratebelief! at the tree's root cluster -> the family sweep (gradient_lg).  The reset, the traversals and the
        root integration are enqueued without host synchronisation; the sweep's fetch is the one wait (the root's constants
        are then copied from a stream that is already idle).  Like loglik_lg, the host mirrors of the beliefs are not
        refreshed.  Returns (loglik, gradient dict): the current site's values, or arrays over the sites (info of a failed
        site is not 0 and its values are NaN) when all_sites."""
        self._ensure_schedule([schedule_tree])
        o = self._opts()
        pa = np.asarray(schedule_tree[-2]).reshape(-1)
        root = int(pa[0]) if pa.size else 0
        _check(self._lib.pgbp_enqueue_calibrate(self._eng, 1, 1, C.byref(o)), self._eng)
        _check(self._lib.pgbp_enqueue_integrate(self._eng, root), self._eng)
        grad = self.gradient_lg(all_sites=True)
        norm = np.zeros(self.n_sites)
        info = np.zeros(self.n_sites, dtype=np.int32)
        _check(self._lib.pgbp_fetch_loglik(self._eng, L.f64p(norm), L.i32p(info)), self._eng)
        grad["info"] = np.where(grad["info"] != 0, grad["info"], info)
        norm = np.where(grad["info"] != 0, np.nan, norm)
        if all_sites:
            return norm, grad
        return float(norm[self.site]), self._gradient_of_site(grad, self.site)

    def gradient_sites_lg(self):
        """pgbp_lg_gradient_sites on the current beliefs: gradient_lg(all_sites=True) for a univariate batch on the
        thread-per-site kernels (p = 1, every belief of at most 2 variables, at least 8 sites; anything else raises
        PGBP_ERR_INVALID), lanes = sites.  The beliefs are read in the layout they are in: nothing is converted, the next
        calibrate_ finds the site-minor layout it left.  Same keys and shapes as gradient_lg(all_sites=True) (dsigma_e when
        tip noise is set, doptima [n_sites, n_regimes, 1] when painted optima are set); the values agree with it to rounding,
        and two calls return the same bytes."""
        nr, n = self._lg_nrates, self.n_sites
        dR = np.zeros((n, nr, 1, 1))
        dmu = np.zeros((n, 1))
        dalpha = np.zeros(n)
        dtheta = np.zeros((n, 1))
        info = np.zeros(n, dtype=np.int32)
        noisy = self.tip_noise_count_lg() > 0
        dsig = np.zeros((n, 1, 1)) if noisy else None
        nopt = self.optima_count_lg()
        if nopt > 0:   # painted optima: pgbp_lg_gradient_sites_optima
            dopt = np.zeros((n, nopt, 1))
            _check(self._lib.pgbp_lg_gradient_sites_optima(self._eng, 0, n, L.f64p(dR), L.f64p(dmu), L.f64p(dalpha),
                                                           L.f64p(dtheta), L.f64p(dsig) if noisy else None, L.f64p(dopt),
                                                           L.i32p(info)), self._eng)
        else:
            _check(self._lib.pgbp_lg_gradient_sites(self._eng, 0, n, L.f64p(dR), L.f64p(dmu), L.f64p(dalpha), L.f64p(dtheta),
                                                    L.f64p(dsig) if noisy else None, L.i32p(info)), self._eng)
        d = dict(dR=dR, dmu=dmu, dalpha=dalpha, dtheta=dtheta, info=info)
        if noisy:
            d["dsigma_e"] = dsig
        if nopt > 0:
            d["doptima"] = dopt
        return d

    def loglik_and_gradient_sites_lg(self, schedule_tree):
        """loglik_and_gradient_lg(schedule_tree, all_sites=True) with the thread-per-site sweep (gradient_sites_lg): beliefs
        reset from the factors -> one calibrate -> integratebelief! at the root cluster -> the sweep, all of it on the
        thread-per-site kernels and in their layout.  Returns (loglik [n_sites], gradient dict); a failed site has info != 0
        and NaN values."""
        self._ensure_schedule([schedule_tree])
        o = self._opts()
        pa = np.asarray(schedule_tree[-2]).reshape(-1)
        root = int(pa[0]) if pa.size else 0
        _check(self._lib.pgbp_enqueue_calibrate(self._eng, 1, 1, C.byref(o)), self._eng)
        _check(self._lib.pgbp_enqueue_integrate(self._eng, root), self._eng)
        grad = self.gradient_sites_lg()
        norm = np.zeros(self.n_sites)
        info = np.zeros(self.n_sites, dtype=np.int32)
        _check(self._lib.pgbp_fetch_loglik(self._eng, L.f64p(norm), L.i32p(info)), self._eng)
        grad["info"] = np.where(grad["info"] != 0, grad["info"], info)
        norm = np.where(grad["info"] != 0, np.nan, norm)
        return norm, grad

    def _loglik_and_sites(self, schedule_tree, sweep, refill=False):
        """the steps of loglik_and_gradient_sites_lg around one of the thread-per-site sweeps (`sweep`: its dict); refill:
        the factors are filled again first, as loglik_and_shift_scan_lg does.  (loglik [n_sites], the sweep's dict, the
        calibration's info [n_sites])"""
        if refill:
            if getattr(self, "_lg_last", None) is None:
                raise L.PgbpError(L.ERR_STATE, "no parameters yet (call assignfactors_lg_ first)")
            m, _keep = self._lg_last
            _check(self._lib.pgbp_lg_assignfactors(self._eng, C.byref(m)), self._eng)
        self._ensure_schedule([schedule_tree])
        o = self._opts()
        pa = np.asarray(schedule_tree[-2]).reshape(-1)
        root = int(pa[0]) if pa.size else 0
        _check(self._lib.pgbp_enqueue_calibrate(self._eng, 1, 1, C.byref(o)), self._eng)
        _check(self._lib.pgbp_enqueue_integrate(self._eng, root), self._eng)
        d = sweep()
        norm = np.zeros(self.n_sites)
        info = np.zeros(self.n_sites, dtype=np.int32)
        _check(self._lib.pgbp_fetch_loglik(self._eng, L.f64p(norm), L.i32p(info)), self._eng)
        return norm, d, info

    def shift_scan_sites_lg(self, min_info=1e-8, information=False, tables=True):
        """pgbp_lg_shift_scan_sites on the current beliefs: shift_scan_lg(all_sites=True) for a univariate batch on the
        thread-per-site kernels (p = 1, every belief of at most 2 variables, at least 8 sites; anything else raises
        PGBP_ERR_INVALID), lanes = sites.  The beliefs are read in the layout they are in: nothing is converted.
        Same keys and [site, family, ...] indexing as shift_scan_lg(all_sites=True) -- jump, lr, dof, identified, edge_jump,
        info, and with information=True H and se = H^-1/2 -- as transposed VIEWS of the call's site-minor rows, not copies;
        the values agree with shift_scan_lg to rounding, and two calls return the same bytes.  Also top_lr [n_sites] and
        top_family [n_sites], formed on the device: the largest lr of each site over the families with an edge that are
        identified and whose lr is finite, and that family (ties to the lowest; -inf and -1 for a site with nothing
        identified; NaN and -1 for a failed site).  tables=False returns only top_lr, top_family and info: no table is
        allocated or fetched."""
        n = self.n_sites
        nf = len(self._lg["cluster"])
        K = self._lg["length"].size // nf if nf else 1
        jump = np.zeros((nf, n)) if tables else None
        lr = np.zeros((nf, n)) if tables else None
        H = np.zeros((nf, n)) if tables and information else None
        top_lr = np.zeros(n)
        top_family = np.zeros(n, dtype=np.int32)
        info = np.zeros(n, dtype=np.int32)
        _check(self._lib.pgbp_lg_shift_scan_sites(self._eng, 0, n, float(min_info), L.f64p(jump) if tables else None,
                                                  L.f64p(lr) if tables else None, L.f64p(H) if H is not None else None,
                                                  L.f64p(top_lr), L.i32p(top_family), L.i32p(info)), self._eng)
        d = dict(top_lr=top_lr, top_family=top_family, info=info)
        if not tables:
            return d
        jump = jump.T[:, :, None]
        bits = ~np.isnan(jump)
        gam = np.asarray(self._lg["gamma"], np.float64).reshape(nf, K)
        real = np.arange(K)[None, :] < np.asarray(self._lg["n_parents"]).reshape(nf, 1)
        inv = np.full((nf, K), np.nan)
        ok = real & (gam != 0.0)
        inv[ok] = 1.0 / gam[ok]
        d.update(jump=jump, lr=lr.T, dof=bits.sum(axis=2).astype(np.int32), identified=bits,
                 edge_jump=jump[:, :, None, :] * inv[None, :, :, None])
        if information:
            d["H"] = H.T[:, :, None, None]
            d["se"] = 1.0 / np.sqrt(H.T[:, :, None])
        return d

    def loglik_and_shift_scan_sites_lg(self, schedule_tree, min_info=1e-8, information=False, tables=True):
        """loglik_and_shift_scan_lg(schedule_tree, all_sites=True) with the thread-per-site scan (shift_scan_sites_lg): the
        factors filled again (so that shifts set since the last assignfactors_lg_ are in) -> one calibrate -> integratebelief!
        at the root cluster -> the scan, all of it on the thread-per-site kernels and in their layout.  Returns
        (loglik [n_sites], scan dict); a failed site has info != 0 and NaN values (top_family -1)."""
        norm, scan, info = self._loglik_and_sites(
            schedule_tree, lambda: self.shift_scan_sites_lg(min_info=min_info, information=information, tables=tables), refill=True)
        scan["info"] = np.where(scan["info"] != 0, scan["info"], info)
        return np.where(scan["info"] != 0, np.nan, norm), scan

    def optimum_scan_sites_lg(self, min_info=1e-8, information=False, tables=True):
        """pgbp_lg_optimum_scan_sites on the current beliefs: every edge scanned for a shift of the optimum of its clade under
        OU, for a univariate batch on a tree on the thread-per-site kernels (the conditions of gradient_sites_lg, a topology
        set, every family with one parent), lanes = sites.  For the edge above family v the increment `delta` is added to the
        optimum of every edge of clade(v), whatever regimes they carry; the painted optima in force are read, so after a
        regime is painted the scan gives the NEXT increment.  Returns a dict: delta, lr [site, family] as transposed views of
        the call's site-minor rows (delta NaN and lr 0 where the family is not identified or skipped; both NaN for a
        root-prior family), with information=True also information (H) and se = H^-1/2; top_lr, top_family [n_sites] formed
        on the device (the largest lr over the identified families that have a parent, ties to the lowest family; -inf and -1
        where nothing is identified; NaN and -1 at a failed site) and info [n_sites].  tables=False returns only top_lr,
        top_family and info: no table is allocated or fetched.  Two calls return the same bytes."""
        n = self.n_sites
        nf = len(self._lg["cluster"])
        delta = np.zeros((nf, n)) if tables else None
        lr = np.zeros((nf, n)) if tables else None
        H = np.zeros((nf, n)) if tables and information else None
        top_lr = np.zeros(n)
        top_family = np.zeros(n, dtype=np.int32)
        info = np.zeros(n, dtype=np.int32)
        _check(self._lib.pgbp_lg_optimum_scan_sites(self._eng, 0, n, float(min_info), L.f64p(delta) if tables else None,
                                                    L.f64p(lr) if tables else None, L.f64p(H) if H is not None else None,
                                                    L.f64p(top_lr), L.i32p(top_family), L.i32p(info)), self._eng)
        d = dict(top_lr=top_lr, top_family=top_family, info=info)
        if not tables:
            return d
        d.update(delta=delta.T, lr=lr.T)
        if information:
            d["information"] = H.T
            d["se"] = 1.0 / np.sqrt(H.T)
        return d

    def loglik_and_optimum_scan_sites_lg(self, schedule_tree, min_info=1e-8, information=False, tables=True):
        """The factors filled again (so that optima, shifts and noise set since the last assignfactors_lg_ are in) -> one
        calibrate -> integratebelief! at the root cluster, enqueued as loglik_and_gradient_sites_lg does -> the sweep of
        optimum_scan_sites_lg.  Returns (loglik [n_sites], scan dict); a failed site has info != 0 and NaN values."""
        norm, scan, info = self._loglik_and_sites(
            schedule_tree, lambda: self.optimum_scan_sites_lg(min_info=min_info, information=information, tables=tables), refill=True)
        scan["info"] = np.where(scan["info"] != 0, scan["info"], info)
        return np.where(scan["info"] != 0, np.nan, norm), scan

    def edge_gradient_sites_lg(self):
        """pgbp_lg_edge_gradient_sites on the current beliefs: edge_gradient_lg(all_sites=True) for a univariate batch on the
        thread-per-site kernels (the conditions of gradient_sites_lg), lanes = sites, nothing converted.  Same keys and
        [site, family, ...] indexing -- dlength, dgamma [n_sites, n_families, K], dshift [n_sites, n_families, 1], info -- as
        transposed views of the call's site-minor rows; the values agree with edge_gradient_lg to rounding, and two calls
        return the same bytes."""
        n = self.n_sites
        nf = len(self._lg["cluster"])
        K = self._lg["length"].size // nf if nf else 1
        dlength = np.zeros((nf, K, n))
        dgamma = np.zeros((nf, K, n))
        dshift = np.zeros((nf, n))
        info = np.zeros(n, dtype=np.int32)
        _check(self._lib.pgbp_lg_edge_gradient_sites(self._eng, 0, n, L.f64p(dlength), L.f64p(dgamma), L.f64p(dshift),
                                                     L.i32p(info)), self._eng)
        return dict(dlength=dlength.transpose(2, 0, 1), dgamma=dgamma.transpose(2, 0, 1), dshift=dshift.T[:, :, None], info=info)

    def loglik_and_edge_gradient_sites_lg(self, schedule_tree):
        """loglik_and_edge_gradient_lg(schedule_tree, all_sites=True) with the thread-per-site sweep (edge_gradient_sites_lg),
        built as loglik_and_gradient_sites_lg is.  Returns (loglik [n_sites], edge-gradient dict); a failed site has
        info != 0 and NaN values."""
        norm, grad, info = self._loglik_and_sites(schedule_tree, self.edge_gradient_sites_lg)
        grad["info"] = np.where(grad["info"] != 0, grad["info"], info)
        return np.where(grad["info"] != 0, np.nan, norm), grad

    def loo_sites_lg(self):
        """pgbp_lg_loo_sites on the current beliefs: loo_lg(all_sites=True) for a univariate batch on the thread-per-site
        kernels (the conditions of gradient_sites_lg), lanes = sites, nothing converted.  Same keys and [site, tip, ...]
        indexing -- families, mean [n_sites, n_tip, 1], cov [n_sites, n_tip, 1, 1], lpd, total, info [n_sites, n_tip], y -- as
        transposed views of the call's site-minor rows.  total adds the tips in another order than loo_lg: the two agree to
        rounding, as every other value; two calls return the same bytes.  A (tip, site) that a per-site mask hides
        (set_site_missing_lg) has NaN values and info -2 (PGBP_INFO_NOT_OBSERVED), and adds nothing to total."""
        nt = int(self._lib.pgbp_lg_loo_count(self._eng))
        if nt < 0:
            _check(self._lib.pgbp_lg_loo_sites(self._eng, 0, 0, None, None, None, None, None), self._eng)
            raise L.PgbpError(L.ERR_STATE, "pgbp_lg_loo_count failed")
        fam = np.zeros(max(nt, 1), dtype=np.int32)
        _check(self._lib.pgbp_lg_loo_families(self._eng, L.i32p(fam)), self._eng)
        fam = fam[:nt]
        n = self.n_sites
        mean = np.zeros((max(nt, 1), n))
        var = np.zeros((max(nt, 1), n))
        lpd = np.zeros((max(nt, 1), n))
        total = np.zeros(n)
        info = np.zeros((max(nt, 1), n), dtype=np.int32)
        _check(self._lib.pgbp_lg_loo_sites(self._eng, 0, n, L.f64p(mean), L.f64p(var), L.f64p(lpd), L.f64p(total), L.i32p(info)),
               self._eng)
        y = self._lg["data"][:, self._lg["data_row"][fam]]
        return dict(families=fam, mean=mean[:nt].T[:, :, None], cov=var[:nt].T[:, :, None, None], lpd=lpd[:nt].T, total=total,
                    info=info[:nt].T, y=y)

    def loo_and_loglik_sites_lg(self, schedule_tree):
        """loo_and_loglik_lg(schedule_tree, all_sites=True) with the thread-per-site sweep (loo_sites_lg), built as
        loglik_and_gradient_sites_lg is.  Returns (loglik [n_sites], loo dict); loglik of a site whose calibration failed is
        NaN."""
        norm, loo, info = self._loglik_and_sites(schedule_tree, self.loo_sites_lg)
        return np.where(info != 0, np.nan, norm), loo

    loglik_and_loo_sites_lg = loo_and_loglik_sites_lg

    def moments_sites_(self, beliefs=None, cov=True):
        """pgbp_moments_sites on the current beliefs: moments_(beliefs, cov, all_sites=True) for a univariate batch on the
        thread-per-site kernels (the conditions of gradient_sites_lg; anything else raises PGBP_ERR_INVALID), lanes = sites,
        nothing converted.  The same list of (mu [n_sites, m], Sigma [n_sites, m, m] or None, norm [n_sites], info [n_sites]):
        mu, norm and info as transposed views of the call's site-minor rows, Sigma expanded from the packed upper triangle.
        The values agree with moments_ to rounding; two calls return the same bytes."""
        if beliefs is None:
            lst = np.arange(self.nclusters, dtype=np.int32)
            ptr, n = None, 0
        else:
            lst = np.ascontiguousarray(beliefs, dtype=np.int32).reshape(-1)
            ptr, n = L.i32p(lst if lst.size else np.zeros(1, dtype=np.int32)), int(lst.size)
        ok = (lst >= 0) & (lst < len(self._dims))
        dims = np.where(ok, self._dims[np.where(ok, lst, 0)], 0).astype(np.int64)   # (the call reports a bad index)
        ns = self.n_sites
        nm, nt, nl = int(dims.sum()), int((dims * (dims + 1) // 2).sum()), int(lst.size)
        mean = np.zeros((max(nm, 1), ns))
        tri = np.zeros((max(nt, 1), ns)) if cov else None
        norm = np.zeros((max(nl, 1), ns))
        info = np.zeros((max(nl, 1), ns), dtype=np.int32)
        _check(self._lib.pgbp_moments_sites(self._eng, n, ptr, 0, ns, L.f64p(mean), L.f64p(tri) if cov else None, L.f64p(norm),
                                            L.i32p(info)), self._eng)
        res, am, at = [], 0, 0
        for i, m in enumerate(int(d) for d in dims):
            Sig = None
            if cov:
                Sig = np.empty((ns, m, m))
                for b in range(m):
                    for a in range(b + 1):
                        Sig[:, a, b] = Sig[:, b, a] = tri[at + b * (b + 1) // 2 + a]
                at += m * (m + 1) // 2
            res.append((mean[am: am + m].T, Sig, norm[i], info[i]))
            am += m
        return res

    def node_moments_sites(self, nodes=None):
        """Posterior mean and variance of the nodes of a univariate batch, lanes = sites: {node label: (mean [n_sites],
        var [n_sites])} from one moments_sites_ call over the first cluster that holds each node (node_samples' rule); NaN for
        a node whose trait is out of scope there and where the cluster's info is not 0.  nodes=None: every labelled node."""
        ent = self._node_entries("node_moments_sites")
        nodes = list(ent) if nodes is None else list(nodes)
        for v in nodes:
            if v not in ent:
                raise ValueError(f"no cluster holds node {v!r}")
        clusters = sorted({ent[v][0] for v in nodes})
        mom = dict(zip(clusters, self.moments_sites_(clusters, cov=True)))
        out = {}
        for v in nodes:
            ci, pos, _ = ent[v]
            if pos[0] < 0:
                out[v] = (np.full(self.n_sites, np.nan), np.full(self.n_sites, np.nan))
            else:
                out[v] = (mom[ci][0][:, pos[0]], mom[ci][1][:, pos[0], pos[0]])
        return out

    def sample_posterior_sites_(self, n_draws=1, z=None, seed=None, schedule_tree=0):
        """pgbp_sample_posterior_sites: sample_posterior_(all_sites=True) for a univariate batch on the thread-per-site kernels
        (the conditions of gradient_sites_lg), lanes = sites, nothing converted.  z: standard normals [n_draws, n_sites, size]
        as sample_posterior_ takes them (copied once into the call's site-minor order), or None: the DEVICE generates them
        from `seed` (Philox4x32-10, the convention of include/pgbp.h; None: a seed drawn from numpy) and nothing is copied up.
        Returns (x, info, views) indexed as sample_posterior_(all_sites=True) -- x [n_draws, n_sites, size], info [n_sites],
        views[i] = x[:, :, cluster i's variables] -- as views of the call's site-minor array [n_draws, size, n_sites], so
        node_samples works unchanged.  The same z gives sample_posterior_'s draws to rounding."""
        size = int(self._lib.pgbp_sample_size(self._eng))
        ns, n_draws = self.n_sites, int(n_draws)
        shape = (max(n_draws, 0), ns, size)
        zp = None
        if z is not None:
            z = np.asarray(z, dtype=np.float64)
            if z.shape != shape:
                raise ValueError(f"z has shape {z.shape}, expected {shape}")
            zs = np.ascontiguousarray(z.transpose(0, 2, 1))
            zp = L.f64p(zs if zs.size else np.zeros(1))
        elif seed is None:
            seed = int(np.random.default_rng().integers(0, 2 ** 63))
        xs = np.zeros((shape[0], size, ns))
        info = np.zeros(ns, dtype=np.int32)
        _check(self._lib.pgbp_sample_posterior_sites(self._eng, int(schedule_tree), 0, ns, n_draws, zp,
                                                     int(seed or 0) & 0xFFFFFFFFFFFFFFFF, L.f64p(xs if xs.size else np.zeros(1)),
                                                     L.i32p(info)), self._eng)
        x = xs.transpose(0, 2, 1)
        off = np.concatenate([[0], np.cumsum(self._dims[: self.nclusters].astype(np.int64))])
        return x, info, [x[:, :, off[i]: off[i + 1]] for i in range(self.nclusters)]

    def posterior_cov_sites_(self, c, schedule_tree=0, want_w=True, want_k=True, want_gram=True):
        """pgbp_posterior_cov_sites: posterior_cov_(all_sites=True) for a univariate batch on the thread-per-site kernels (the
        conditions of gradient_sites_lg), lanes = sites, nothing converted, plus the Gram matrix of the columns folded on the
        device.  c: [n_cols, size] (or [size]), shared by the sites.
        Returns (w, k, gram, info): w and k indexed as posterior_cov_(all_sites=True) -- [n_cols, n_sites, size] -- as
        transposed views of the call's site-minor rows; gram [n_sites, n_cols, n_cols], gram[s, a, b] = w_a . w_b =
        Cov(c_a'x, c_b'x | data) at site s, expanded from the packed upper triangle; info [n_sites] as sample_posterior_sites_'
        (a site whose info is not 0 is NaN in all three).  want_* false: that array is None and is neither computed beyond
        what the others need nor moved -- with only gram no table of size x sites exists on the host.  The values agree with
        posterior_cov_ to rounding; two calls return the same bytes."""
        size = int(self._lib.pgbp_sample_size(self._eng))
        ns = self.n_sites
        c = np.ascontiguousarray(np.atleast_2d(np.asarray(c, dtype=np.float64)))
        if c.ndim != 2 or c.shape[1] != size:
            raise ValueError(f"c has shape {c.shape}, expected (n_cols, {size})")
        nc = int(c.shape[0])
        ws = np.zeros((nc, size, ns)) if want_w else None
        ks = np.zeros((nc, size, ns)) if want_k else None
        tri = np.zeros((max(nc * (nc + 1) // 2, 1), ns)) if want_gram else None
        info = np.zeros(ns, dtype=np.int32)
        ptr = lambda a: None if a is None else L.f64p(a if a.size else np.zeros(1))
        _check(self._lib.pgbp_posterior_cov_sites(self._eng, int(schedule_tree), 0, ns, nc, L.f64p(c if c.size else np.zeros(1)),
                                                  ptr(ws), ptr(ks), ptr(tri), L.i32p(info)), self._eng)
        gram = None
        if want_gram:
            gram = np.empty((ns, nc, nc))
            for b in range(nc):
                for a in range(b + 1):
                    gram[:, a, b] = gram[:, b, a] = tri[b * (b + 1) // 2 + a]
        tr = lambda a: None if a is None else a.transpose(0, 2, 1)
        return tr(ws), tr(ks), gram, info

    def node_cov_sites(self, nodes_a, nodes_b=None, schedule_tree=0):
        """Posterior covariance between nodes that need not share a cluster, at every site of a univariate batch:
        [n_sites, len(a), len(b)], entry [s, i, j] = Cov(a_i, b_j | data) at site s; nodes_b=None: nodes_a among themselves.
        One column of posterior_cov_sites_ per in-scope node of b, node_cov's rule for the cluster that holds a node.  NaN for
        a node whose trait is out of scope and at a site whose info is not 0 -- it does not raise: one bad site must not hide
        the others."""
        ent = self._node_entries("node_cov_sites")
        nodes_a = list(nodes_a)
        nodes_b = nodes_a if nodes_b is None else list(nodes_b)
        for v in nodes_a + nodes_b:
            if v not in ent:
                raise ValueError(f"no cluster holds node {v!r}")
        size = int(self._lib.pgbp_sample_size(self._eng))
        cols = [(j, int(ent[v][2][0])) for j, v in enumerate(nodes_b) if ent[v][2][0] >= 0]
        out = np.full((self.n_sites, len(nodes_a), len(nodes_b)), np.nan)
        if not cols or not nodes_a:
            return out
        c = np.zeros((len(cols), size))
        c[np.arange(len(cols)), [e for _, e in cols]] = 1.0
        _, k, _, _ = self.posterior_cov_sites_(c, schedule_tree, want_w=False, want_gram=False)
        for i, v in enumerate(nodes_a):
            ea = int(ent[v][2][0])
            if ea >= 0:
                for q, (j, _) in enumerate(cols):
                    out[:, i, j] = k[q, :, ea]
        return out

    def functional_moments_sites(self, weights, schedule_tree=0):
        """Posterior mean [n_sites, q] and covariance [n_sites, q, q] of the q linear functionals sum_v W_v x_v at every site
        of a univariate batch; weights: {node label: W_v [q] or [q, 1]}.  The covariance is the device's gram of
        posterior_cov_sites_ alone (no table is fetched), the mean comes from moments_sites_ without the covariance.  A
        non-zero weight on a trait out of scope is refused, as functional_moments does; a site whose info is not 0 is NaN."""
        ent = self._node_entries("functional_moments_sites")
        nodes = list(weights)
        size = int(self._lib.pgbp_sample_size(self._eng))
        W = [np.asarray(weights[v], dtype=np.float64).reshape(-1, 1) for v in nodes]
        q = W[0].shape[0] if W else 0
        c = np.zeros((q, size))
        for v, Wv in zip(nodes, W):
            if v not in ent:
                raise ValueError(f"no cluster holds node {v!r}")
            e = ent[v][2]
            if Wv.shape != (q, len(e)):
                raise ValueError(f"the weights of node {v!r} have shape {Wv.shape}, expected {(q, len(e))}")
            if np.any(Wv[:, e < 0] != 0.0):
                raise ValueError(f"node {v!r}: weight on a trait that is out of scope")
            c[:, e[e >= 0]] += Wv[:, e >= 0]
        ns = self.n_sites
        if q == 0:
            return np.zeros((ns, 0)), np.zeros((ns, 0, 0))
        _, _, gram, _ = self.posterior_cov_sites_(c, schedule_tree, want_w=False, want_k=False)
        held = [v for v in nodes if ent[v][1][0] >= 0]
        clusters = sorted({ent[v][0] for v in held})
        mom = dict(zip(clusters, self.moments_sites_(clusters, cov=False))) if clusters else {}
        mean = np.zeros((ns, q))
        for v, Wv in zip(nodes, W):
            ci, pos, _ = ent[v]
            if pos[0] >= 0:
                with np.errstate(invalid="ignore"):   # (a failed site: Inf or NaN times a zero weight; NaN below)
                    mean = mean + mom[ci][0][:, pos[0]][:, None] * Wv[:, 0][None, :]
        return np.where(np.isnan(gram[:, np.arange(q), np.arange(q)]), np.nan, mean), gram

    def impute_sites_lg(self):
        """pgbp_lg_impute_sites on the current beliefs: impute_lg(all_sites=True) for a univariate batch on the thread-per-site
        kernels (the conditions of gradient_sites_lg), lanes = sites, nothing converted.  Same keys and [site, tip, ...]
        indexing -- families, rows, predicted [n, 1], mean [n_sites, n, 1], cov [n_sites, n, 1, 1], info [n_sites, n] -- as
        transposed views of the call's site-minor rows, so imputed_data takes a site of it; the values agree with impute_lg
        to rounding, and two calls return the same bytes.  With a per-site mask in force (set_site_missing_lg) the list also
        holds every tip masked at some site: predicted where it is masked, NaN with info -2 (PGBP_INFO_NOT_OBSERVED) where it
        is observed."""
        n = int(self._lib.pgbp_lg_impute_count(self._eng))
        if n < 0:
            _check(self._lib.pgbp_lg_impute_sites(self._eng, 0, 0, None, None, None), self._eng)
            raise L.PgbpError(L.ERR_STATE, "pgbp_lg_impute_count failed")
        fam = np.zeros(max(n, 1), dtype=np.int32)
        pred = np.zeros(max(n, 1), dtype=np.uint64)
        _check(self._lib.pgbp_lg_impute_families(self._eng, L.i32p(fam), pred.ctypes.data_as(C.POINTER(C.c_uint64))), self._eng)
        fam, pred = fam[:n], pred[:n]
        ns = self.n_sites
        mean = np.full((max(n, 1), ns), np.nan)
        var = np.full((max(n, 1), ns), np.nan)
        info = np.zeros((max(n, 1), ns), dtype=np.int32)
        _check(self._lib.pgbp_lg_impute_sites(self._eng, 0, ns, L.f64p(mean), L.f64p(var), L.i32p(info)), self._eng)
        return dict(families=fam, rows=self._lg["data_row"][fam], predicted=(pred & np.uint64(1)).astype(bool).reshape(n, 1),
                    mean=mean[:n].T[:, :, None], cov=var[:n].T[:, :, None, None], info=info[:n].T)

    def impute_and_loglik_sites_lg(self, schedule_tree):
        """impute_and_loglik_lg(schedule_tree, all_sites=True) with the thread-per-site sweep (impute_sites_lg), built as
        loglik_and_gradient_sites_lg is.  Returns (loglik [n_sites], impute dict); loglik of a site whose calibration failed
        is NaN."""
        norm, imp, info = self._loglik_and_sites(schedule_tree, self.impute_sites_lg)
        return np.where(info != 0, np.nan, norm), imp

    def edge_gradient_lg(self, all_sites=False):
        """pgbp_lg_edge_gradient on the current beliefs: the derivative of the log-likelihood in every edge length, in every
        inheritance and in a shift of the mean on every edge, under the parameters of the last assignfactors_lg_ -- one sweep
        over the node families, each family writing its own numbers.  EXACT ONLY when the beliefs are calibrated (postorder
        and preorder) on a clique tree under those parameters (not verified), as gradient_lg.
        Returns a dict: dlength, dgamma [n_families, K] (K = max_parents, the per-parent order of the family table given to
        lg_setup; NaN where a family has no such edge; dgamma is the FREE partial in each gamma: at gamma_minor =
        1 - gamma_major the derivative in gamma_major is dgamma[major] - dgamma[minor]), dshift [n_families, p] (the score of
        an additive shift of the child's conditional mean; a root-prior family: its dmu term) and info; with a leading site
        axis when all_sites.  A site whose info is not 0 holds NaN; for the current site that raises."""
        p = self._lg_p
        nf = len(self._lg["cluster"])
        K = self._lg["length"].size // nf if nf else 1
        s0, s1 = (0, self.n_sites) if all_sites else (self.site, self.site + 1)
        n = s1 - s0
        dlength = np.zeros((n, nf, K))
        dgamma = np.zeros((n, nf, K))
        dshift = np.zeros((n, nf, p))
        info = np.zeros(n, dtype=np.int32)
        _check(self._lib.pgbp_lg_edge_gradient(self._eng, s0, s1, L.f64p(dlength), L.f64p(dgamma), L.f64p(dshift),
                                               L.i32p(info)), self._eng)
        d = dict(dlength=dlength, dgamma=dgamma, dshift=dshift, info=info)
        return d if all_sites else self._edge_gradient_of_site(d, 0)

    @staticmethod
    def _edge_gradient_of_site(d, s):
        if d["info"][s]:
            raise np.linalg.LinAlgError(f"PosDefException: belief {d['info'][s] - 1} is not positive definite")
        return dict(dlength=d["dlength"][s].copy(), dgamma=d["dgamma"][s].copy(), dshift=d["dshift"][s].copy(), info=0)

    def loglik_and_edge_gradient_lg(self, schedule_tree, all_sites=False):
        """Log-likelihood and its derivatives in every edge under the parameters of the last assignfactors_lg_ on a clique
        tree: the steps of loglik_and_gradient_lg with the edge sweep (edge_gradient_lg) in place of the parameter sweep.
        Returns (loglik, edge-gradient dict): the current site's values, or arrays over the sites (info of a failed site is
        not 0 and its values are NaN) when all_sites."""
        self._ensure_schedule([schedule_tree])
        o = self._opts()
        pa = np.asarray(schedule_tree[-2]).reshape(-1)
        root = int(pa[0]) if pa.size else 0
        _check(self._lib.pgbp_enqueue_calibrate(self._eng, 1, 1, C.byref(o)), self._eng)
        _check(self._lib.pgbp_enqueue_integrate(self._eng, root), self._eng)
        grad = self.edge_gradient_lg(all_sites=True)
        norm = np.zeros(self.n_sites)
        info = np.zeros(self.n_sites, dtype=np.int32)
        _check(self._lib.pgbp_fetch_loglik(self._eng, L.f64p(norm), L.i32p(info)), self._eng)
        grad["info"] = np.where(grad["info"] != 0, grad["info"], info)
        norm = np.where(grad["info"] != 0, np.nan, norm)
        if all_sites:
            return norm, grad
        return float(norm[self.site]), self._edge_gradient_of_site(grad, self.site)

    def set_edges_lg(self, length=None, gamma=None):
        """pgbp_lg_set_edges: replace the edge lengths and / or inheritances of the family table given to lg_setup
        ([n_families * K] each, the table's own layout; None: left as it is) on the device, without uploading the data
        again.  The next assignfactors_lg_ or loglik_lg uses them; beliefs and factors are not refilled by this call."""
        nk = self._lg["length"].size
        arr = {}
        for name, v in (("length", length), ("gamma", gamma)):
            if v is not None:
                arr[name] = np.ascontiguousarray(np.asarray(v, np.float64).reshape(-1))
                assert arr[name].size == nk, name
        _check(self._lib.pgbp_lg_set_edges(self._eng, L.f64p(arr["length"]) if "length" in arr else None,
                                           L.f64p(arr["gamma"]) if "gamma" in arr else None), self._eng)
        self._lg.update(arr)

    def _shift_edges(self, edges):
        """(family, k) pairs or flat indices family * K + k -> flat int32 indices."""
        nf = len(self._lg["cluster"])
        K = self._lg["length"].size // nf if nf else 1
        e = np.asarray(edges, np.int64)
        if e.ndim == 2:
            if e.shape[1] != 2:
                raise ValueError("edges: (family, k) pairs or flat indices family * K + k")
            if e.size and (e[:, 1].min() < 0 or e[:, 1].max() >= K):
                raise ValueError(f"edges: k must be in 0 .. {K - 1}")
            e = e[:, 0] * K + e[:, 1]
        return np.ascontiguousarray(e.reshape(-1), np.int32)

    def set_shifts_lg(self, edges, values):
        """pgbp_lg_set_shifts: mean shifts on edges (the reference's HeterogeneousShiftedBrownianMotion, and the same
        displacement under OU).  edges: (family, k) pairs -- k the parent edge in the per-parent order of the family table
        given to lg_setup -- or flat indices family * K + k; values: [n, p], or [n_sites, n, p] for one set per site.  The
        child's conditional mean gains sum_k gamma_k s_k; a component of a shift outside the family's child_mask has no
        effect.  The call REPLACES the previous shifts (an empty list clears them); the next assignfactors_lg_ or loglik_lg
        uses them, beliefs and factors are not refilled by this call.  The four sweeps (gradient_lg, edge_gradient_lg,
        loo_lg, impute_lg) read the current shifts: call them on beliefs calibrated under them.  An invalid entry raises
        and leaves the previous shifts in force."""
        e = self._shift_edges(edges)
        p = self._lg_p
        v = np.asarray(values, np.float64)
        per_site = v.ndim == 3
        v = np.ascontiguousarray(v.reshape((self.n_sites, e.size, p) if per_site else (e.size, p)))
        _check(self._lib.pgbp_lg_set_shifts(self._eng, int(e.size), L.i32p(e) if e.size else None,
                                            L.f64p(v) if e.size else None, int(per_site)), self._eng)
        self._lg_shift_edges = e

    def clear_shifts_lg(self):
        """Remove every mean shift (pgbp_lg_set_shifts with an empty list)."""
        _check(self._lib.pgbp_lg_set_shifts(self._eng, 0, None, None, 0), self._eng)
        self._lg_shift_edges = np.zeros(0, np.int32)

    def shift_count_lg(self):
        """pgbp_lg_shift_count: the number of shifts in force (0: none)."""
        return int(self._lib.pgbp_lg_shift_count(self._eng))

    def set_optima_lg(self, regime, values):
        """pgbp_lg_set_optima: optima painted on the edges under OU (Hansen's model), as `color` paints the rates.  regime:
        the dense int map [n_families, K] (or flat [n_families * K]; 0 = the edge keeps theta of assignfactors_lg_, r >= 1 =
        its optimum is values[r - 1]; entries of a root-prior family and of k >= n_parents are ignored), or a dict
        {edge: r} with edge a (family, k) pair or a flat index family * K + k (every other edge 0).  values: [n_regimes, p]
        ([n_regimes] at p = 1), or [n_sites, n_regimes, p] for one set per site.  The offset of a family becomes
        sum_k wc_k theta_{r(f,k)}; variances, J, qc and vc are untouched, and under BM (wc = 0) nothing changes.  The call
        REPLACES the previous setting (no values clears it); the next assignfactors_lg_ or loglik_lg uses it, beliefs and
        factors are not refilled by this call.  gradient_lg and gradient_sites_lg honour the optima and return doptima.  The
        other sweeps that form the offsets themselves (edge_gradient_lg, shift_scan_lg, loo_lg, impute_lg, simulate_lg and
        their _sites forms) raise under OU while optima are in force; moments, samples and posterior covariances read
        beliefs only.  An invalid entry raises and leaves the previous optima in force."""
        nf = len(self._lg["cluster"])
        K = self._lg["length"].size // nf if nf else 1
        p = self._lg_p
        if isinstance(regime, dict):
            m = np.zeros(max(1, nf * K), np.int32)
            for edge, r in regime.items():
                m[int(self._shift_edges([edge])[0])] = int(r)
        else:
            m = np.ascontiguousarray(np.asarray(regime, np.int64).reshape(-1), np.int32)
            if m.size != nf * K:
                raise ValueError(f"regime: {nf * K} entries (n_families * K) expected, got {m.size}")
        v = np.asarray(values, np.float64)
        per_site = v.ndim == 3
        n = int(v.shape[1] if per_site else (v.shape[0] if v.ndim else 1)) if v.size else 0
        if n == 0:
            return self.clear_optima_lg()
        v = np.ascontiguousarray(v.reshape((self.n_sites, n, p) if per_site else (n, p)))
        _check(self._lib.pgbp_lg_set_optima(self._eng, n, L.i32p(m), L.f64p(v), int(per_site)), self._eng)
        self._lg_optima = dict(regime=m.reshape(nf, K).copy(), values=v.copy(), per_site=bool(per_site))

    def update_optima_lg(self, values):
        """pgbp_lg_update_optima: new values for the optima in force, in the shape set_optima_lg was given; the regime map
        and the device buffers stay (what fit_sites_lg does at every step).  Takes effect at the next fill; a value that is
        not finite raises and leaves the previous values in force."""
        o = getattr(self, "_lg_optima", None)
        if o is None:
            raise L.PgbpError(L.ERR_STATE, "no optima are set (call set_optima_lg first)")
        v = np.ascontiguousarray(np.asarray(values, np.float64).reshape(o["values"].shape))
        _check(self._lib.pgbp_lg_update_optima(self._eng, L.f64p(v)), self._eng)
        o["values"] = v.copy()

    def clear_optima_lg(self):
        """Remove the painted optima (pgbp_lg_set_optima with no regime)."""
        _check(self._lib.pgbp_lg_set_optima(self._eng, 0, None, None, 0), self._eng)
        self._lg_optima = None

    def optima_lg(self):
        """The painted optima in force: None, or a dict with regime [n_families, K], values [n_regimes, p] (or
        [n_sites, n_regimes, p]) and per_site -- copies of what set_optima_lg was given."""
        o = getattr(self, "_lg_optima", None)
        if o is None or self.optima_count_lg() == 0:
            return None
        return dict(regime=o["regime"].copy(), values=o["values"].copy(), per_site=o["per_site"])

    def optima_count_lg(self):
        """pgbp_lg_optima_count: the number of regimes in force (0: none)."""
        return int(self._lib.pgbp_lg_optima_count(self._eng))

    def set_clade_shifts_sites_lg(self, family, delta):
        """pgbp_lg_set_clade_shifts_sites: per-site clade shifts of the OU optimum, the nested-shift parametrisation that
        optimum_scan_sites_lg scans.  family: int [n_slots, n_sites] (a flat [n_sites] is one slot), -1 = an empty slot;
        delta: float of the same shape.  At site s the optimum of every edge of clade(family[j, s]) -- that family's parent
        edge and every edge below it -- gains delta[j, s], on top of theta or the painted value.  Accepted only on a
        thread-per-site engine (p = 1, every belief of at most 2 variables, at least 8 sites) on a tree with set_topology_lg
        done.  The call REPLACES the previous setting (no slots clears it); the next assignfactors_lg_ or loglik_lg uses it.
        The fill, loglik_lg and optimum_scan_sites_lg honour it; moments, samples and posterior covariances read beliefs
        only; every sweep that raises under painted optima, and gradient_lg / gradient_sites_lg, raise under OU while it is
        in force.  Under BM it has no effect.  An invalid entry (a family out of range, a root-prior family, a family twice
        at one site, a delta that is not finite) raises and leaves the previous setting in force."""
        fam = np.asarray(family, np.int64)
        if fam.ndim == 1:
            fam = fam.reshape(1, -1)
        n_slots = int(fam.shape[0]) if fam.size else 0
        if n_slots == 0:
            return self.clear_clade_shifts_sites_lg()
        if fam.shape != (n_slots, self.n_sites):
            raise ValueError(f"family: [n_slots, {self.n_sites}] expected, got {fam.shape}")
        fam = np.ascontiguousarray(fam, np.int32)
        d = np.ascontiguousarray(np.asarray(delta, np.float64).reshape(n_slots, self.n_sites))
        _check(self._lib.pgbp_lg_set_clade_shifts_sites(self._eng, n_slots, L.i32p(fam), L.f64p(d)), self._eng)

    def update_clade_shifts_sites_lg(self, delta):
        """pgbp_lg_update_clade_shifts_sites: new deltas [n_slots, n_sites] for the families in force; nothing is allocated
        and the families are not checked again (what fit_clade_shifts_sites_lg does at every step).  Takes effect at the
        next fill; a delta that is not finite raises and leaves the previous values in force."""
        n_slots = self.clade_shift_slots_lg()
        if n_slots <= 0:
            raise L.PgbpError(L.ERR_STATE, "no clade shifts are set (call set_clade_shifts_sites_lg first)")
        d = np.ascontiguousarray(np.asarray(delta, np.float64).reshape(n_slots, self.n_sites))
        _check(self._lib.pgbp_lg_update_clade_shifts_sites(self._eng, L.f64p(d)), self._eng)

    def clear_clade_shifts_sites_lg(self):
        """Remove the per-site clade shifts (pgbp_lg_set_clade_shifts_sites with no slot)."""
        _check(self._lib.pgbp_lg_set_clade_shifts_sites(self._eng, 0, None, None), self._eng)

    def clade_shift_slots_lg(self):
        """pgbp_lg_clade_shift_slots: the number of slots in force (0: none)."""
        return int(self._lib.pgbp_lg_clade_shift_slots(self._eng))

    def clade_shifts_sites_lg(self):
        """The per-site clade shifts in force: None, or a dict with family int32 [n_slots, n_sites] (-1: empty) and delta
        [n_slots, n_sites] (0 at an empty slot), as the engine holds them."""
        n_slots = self.clade_shift_slots_lg()
        if n_slots <= 0:
            return None
        fam = np.zeros((n_slots, self.n_sites), np.int32)
        d = np.zeros((n_slots, self.n_sites))
        _check(self._lib.pgbp_lg_get_clade_shifts_sites(self._eng, L.i32p(fam), L.f64p(d)), self._eng)
        return dict(family=fam, delta=d)

    def clade_shift_score_sites_lg(self, min_info=1e-8):
        """pgbp_lg_clade_shift_score_sites on the current beliefs: for every slot of every site the score g (the exact
        derivative of the log-likelihood in that delta), the information H (the diagonal of the joint information) and Kt
        of optimum_scan_sites_lg at the site's own family, picked on the device -- no [family, site] table is fetched.
        Returns a dict: g, information, kt [n_slots, n_sites], identified (H finite) and info [n_sites].  An empty slot and
        a failed site are NaN; a slot with H <= min_info Kt has NaN information, as the scan reports it."""
        n_slots = self.clade_shift_slots_lg()
        if n_slots <= 0:
            raise L.PgbpError(L.ERR_STATE, "no clade shifts are set (call set_clade_shifts_sites_lg first)")
        n = self.n_sites
        g = np.zeros((n_slots, n))
        H = np.zeros((n_slots, n))
        kt = np.zeros((n_slots, n))
        info = np.zeros(n, dtype=np.int32)
        _check(self._lib.pgbp_lg_clade_shift_score_sites(self._eng, 0, n, float(min_info), L.f64p(g), L.f64p(H), L.f64p(kt),
                                                         L.i32p(info)), self._eng)
        return dict(g=g, information=H, kt=kt, identified=np.isfinite(H), info=info)

    def loglik_and_clade_shift_score_sites_lg(self, schedule_tree, min_info=1e-8):
        """The factors filled again (so that the deltas set since the last fill are in) -> one calibrate -> integratebelief!
        at the root cluster, enqueued as loglik_and_gradient_sites_lg does -> clade_shift_score_sites_lg.  Returns
        (loglik [n_sites], score dict); a failed site has info != 0 and NaN values."""
        norm, sc, info = self._loglik_and_sites(schedule_tree, lambda: self.clade_shift_score_sites_lg(min_info=min_info), refill=True)
        sc["info"] = np.where(sc["info"] != 0, sc["info"], info)
        return np.where(sc["info"] != 0, np.nan, norm), sc

    def set_tip_noise_lg(self, families, sigma_e, scale=None, se2=None):
        """pgbp_lg_set_tip_noise: measurement error at the tips.  The conditional variance of every listed tip family f
        (child_pos < 0 with a data row) gains E_f = scale_f * sigma_e + diag(se2_f): the tip's data row is then an
        observation y = x + eps of the trait.  families: indices into the family table given to lg_setup; sigma_e: [p, p]
        symmetric (the within-species covariance), or [n_sites, p, p] for one per site; scale: [n] >= 0 (default 1, for
        example 1 / n_f); se2: None or known sampling variances [n, p] >= 0, [n_sites, n, p] with a per-site sigma_e (a
        shared se2 is then repeated).  The call REPLACES the previous noise (an empty list clears it); the next
        assignfactors_lg_ or loglik_lg uses it, beliefs and factors are not refilled by this call.  The sweeps read the
        current noise: loo_lg and impute_lg then predict the OBSERVATION of a noisy tip (variance V + E).  An invalid
        entry raises and leaves the previous noise in force.  Accuracy: a relative error of about 2^-52 (1 + |E| / |V|)
        in a noisy tip's factor (1e-8 at |E| / |V| = 1e7)."""
        p = self._lg_p
        fam = np.ascontiguousarray(np.asarray(families, np.int64).reshape(-1), np.int32)
        n = int(fam.size)
        sig = np.asarray(sigma_e, np.float64)
        per_site = sig.ndim == 3
        sig = np.ascontiguousarray(sig.reshape((self.n_sites, p, p) if per_site else (p, p)))
        sc = np.ascontiguousarray(np.broadcast_to(np.asarray(1.0 if scale is None else scale, np.float64).reshape(-1), (n,)))
        s2 = None
        if se2 is not None:
            s2 = np.asarray(se2, np.float64)
            if per_site:
                s2 = np.broadcast_to(s2.reshape((-1, n, p)), (self.n_sites, n, p))
            else:
                s2 = s2.reshape(n, p)
            s2 = np.ascontiguousarray(s2)
        _check(self._lib.pgbp_lg_set_tip_noise(self._eng, n, L.i32p(fam) if n else None, L.f64p(sc) if n else None,
                                               L.f64p(sig) if n else None, L.f64p(s2) if (n and s2 is not None) else None,
                                               int(per_site)), self._eng)
        self._lg_noise = dict(families=fam, per_site=per_site, scale=sc, se2=s2) if n else None

    def clear_tip_noise_lg(self):
        """Remove the tip noise (pgbp_lg_set_tip_noise with an empty list)."""
        _check(self._lib.pgbp_lg_set_tip_noise(self._eng, 0, None, None, None, None, 0), self._eng)
        self._lg_noise = None

    def tip_noise_count_lg(self):
        """pgbp_lg_tip_noise_count: the number of noisy tips in force (0: none)."""
        return int(self._lib.pgbp_lg_tip_noise_count(self._eng))

    def set_site_missing_lg(self, mask, data=None):
        """pgbp_lg_set_site_missing: per-site missing tips of a univariate batch.  mask: bool [n_sites, n_rows], True = the
        tip with that data row is NOT observed at that site; None clears the mask; "nan": the mask is taken from the NaNs
        of `data` when given, else of the data last given to lg_setup / set_data_lg.  data (optional, [n_sites, n_rows] or
        [n_sites, n_rows, 1]): installed by set_data_lg once the mask is in force, so a table with NaNs at its gaps goes in
        with one call (split_missing_data gives the finite table lg_setup wants first).  Accepted only on a thread-per-site
        engine (p = 1, every belief of at most 2 variables, at least 8 sites; pgbp_patterns otherwise).  The call REPLACES
        the previous mask; the next assignfactors_lg_ or loglik_lg uses it, beliefs and factors are not refilled by this
        call.  The lanes-are-sites sweeps (gradient_sites_lg, shift_scan_sites_lg, edge_gradient_sites_lg, loo_sites_lg,
        impute_sites_lg) read it; the general sweeps raise while it is in force.  A row without a tip, a tip the set-up's
        child_mask already skips, or a site left with nothing observed raises and leaves the previous mask in force.
        UNCOVERED ENTRIES: the device keeps 0.0 at every entry a mask has covered (the value there is never used).  A new
        mask -- or None -- that no longer covers such an entry would make that 0.0 an observed value and the likelihood
        silently wrong, so this wrapper raises ValueError, with nothing changed, unless `data` comes with the call (the C
        call itself leaves this to its caller; include/pgbp.h).
        mask="nan" without `data` reads the NaNs of what lg_setup or set_data_lg were last given: lg_setup takes no NaN
        without a child_mask, so after a complete-data set-up that pattern is empty until set_data_lg has been given NaNs
        under a mask -- pass the table as `data` instead."""
        rows = int(self._lg["data"].shape[1])
        if isinstance(mask, str) and mask == "nan" and data is None and self._lg_data_nan is None:
            raise ValueError("set_site_missing_lg: mask='nan' but no data have been given")
        old = getattr(self, "_lg_site_mask", None)
        if old is not None and data is None:
            if mask is None:
                new = np.zeros_like(old)
            elif isinstance(mask, str):
                new = self._lg_data_nan if mask == "nan" else None
            else:
                new = np.asarray(mask).reshape(self.n_sites, rows) != 0
            if new is not None and (old & ~new).any():
                s_, r_ = np.argwhere(old & ~new)[0]
                raise ValueError(f"set_site_missing_lg: {int((old & ~new).sum())} entries the mask in force covers (the first: site "
                                 f"{int(s_)}, row {int(r_)}) would be uncovered and hold the 0.0 stored there; give `data` with the call")
        if mask is None:
            _check(self._lib.pgbp_lg_set_site_missing(self._eng, None), self._eng)
            self._lg_site_mask = None
        else:
            if isinstance(mask, str):
                if mask != "nan":
                    raise ValueError("set_site_missing_lg: mask is a bool array, None or 'nan'")
                src = self._lg_data_nan if data is None else np.isnan(np.asarray(data, np.float64).reshape(self.n_sites, rows))
                if src is None:
                    raise ValueError("set_site_missing_lg: mask='nan' but no data have been given")
                mask = src
            m = np.ascontiguousarray(np.asarray(mask).reshape(self.n_sites, rows) != 0, np.uint8)
            _check(self._lib.pgbp_lg_set_site_missing(self._eng, m.ctypes.data_as(C.POINTER(C.c_uint8))), self._eng)
            self._lg_site_mask = m.astype(bool) if m.any() else None
        if data is not None:
            self.set_data_lg(np.asarray(data, np.float64).reshape(self.n_sites, rows, 1))

    def site_missing_lg(self):
        """pgbp_lg_get_site_missing: the mask in force, bool [n_sites, n_rows]; all False when none is set."""
        rows = int(self._lg["data"].shape[1])
        m = np.zeros((self.n_sites, max(rows, 1)), np.uint8)
        _check(self._lib.pgbp_lg_get_site_missing(self._eng, m.ctypes.data_as(C.POINTER(C.c_uint8))), self._eng)
        return m.reshape(-1)[: self.n_sites * rows].reshape(self.n_sites, rows).astype(bool)

    def site_missing_count_lg(self):
        """pgbp_lg_site_missing_count: the number of masked (row, site) pairs (0: no mask)."""
        return int(self._lib.pgbp_lg_site_missing_count(self._eng))

    def set_data_lg(self, data, all_sites=True):
        """pgbp_lg_set_data: replace the tip data given to lg_setup -- [n_sites, n_rows, p] (or [n_rows, p] on a one-site
        object; all_sites=False: [n_rows, p] or [1, n_rows, p] for the current site) -- without a new set-up.  The
        missing-data pattern stays the set-up's: an entry outside a tip's mask is ignored (NaN allowed), one inside it that is
        not finite raises and leaves the data as they were.  The next assignfactors_lg_ or loglik_lg uses the new data;
        beliefs and factors are not refilled by this call.  With a per-site mask in force (set_site_missing_lg) an entry
        it masks may hold anything, NaN included; the device stores 0 there."""
        s0, s1 = (0, self.n_sites) if all_sites else (self.site, self.site + 1)
        rows = int(self._lg["data"].shape[1])
        d = np.ascontiguousarray(np.asarray(data, np.float64).reshape(s1 - s0, rows, self._lg_p))
        _check(self._lib.pgbp_lg_set_data(self._eng, s0, s1, L.f64p(d if d.size else np.zeros(1))), self._eng)
        if self._lg_p == 1 and self._lg_data_nan is not None:   # (what set_site_missing_lg("nan") reads)
            self._lg_data_nan[s0:s1] = np.isnan(d[:, :, 0])

    def get_data_lg(self):
        """pgbp_lg_get_data: the tip data the device holds, [n_sites, n_rows, p] (what lg_setup, set_data_lg or
        simulate_lg(write_data=True) left; an entry outside a tip's mask that was not finite reads 0)."""
        rows = int(self._lg["data"].shape[1])
        d = np.zeros((self.n_sites, rows, self._lg_p))
        _check(self._lib.pgbp_lg_get_data(self._eng, 0, self.n_sites, L.f64p(d if d.size else np.zeros(1))), self._eng)
        return d

    def simulate_lg(self, z=None, seed=None, write_data=False, all_sites=False, return_z=False):
        """pgbp_lg_simulate: every node of the network drawn from the CURRENT model -- the parameters of the last
        assignfactors_lg_, the edges, shifts and tip noise in force -- in one device sweep; sites are replicates.
        Exactly one of z and seed: z = standard normals [n_sites or 1, n_families, p] (z = 0 gives the prior means, a
        caller can reproduce a draw from z: include/pgbp.h has the recipe), or seed = an integer < 2^64 for the device's own
        stateless generator (Philox4x32-10 + Box-Muller: the draw of a (site, family, trait) depends on nothing else).
        write_data: the tips' observed traits go straight into the engine's data, as set_data_lg would put them; the next
        assignfactors_lg_ or loglik_lg uses them.  Needs the family table's `parent_family` (factors.lg_families gives it)
        and a fixed root or a proper root prior.
        Returns (x, info) -- with return_z (x, info, z) --: x [n_sites or 1, n_families, p], family order (a noisy tip's row
        is its OBSERVATION); info [n_sites or 1]: 0, or the 1-based index of the first family whose conditional variance is
        not positive definite (that site's x is NaN, its data untouched)."""
        if (z is None) == (seed is None):
            raise ValueError("simulate_lg takes exactly one of z and seed")
        s0, s1 = (0, self.n_sites) if all_sites else (self.site, self.site + 1)
        shape = (s1 - s0, len(self._lg["cluster"]), self._lg_p)
        if z is not None:
            z = np.ascontiguousarray(z, dtype=np.float64)
            if z.shape != shape:
                raise ValueError(f"z has shape {z.shape}, expected {shape}")
        x = np.zeros(shape)
        zo = np.zeros(shape) if return_z else None
        info = np.zeros(s1 - s0, dtype=np.int32)
        ptr = lambda a: None if a is None else L.f64p(a if a.size else np.zeros(1))
        _check(self._lib.pgbp_lg_simulate(self._eng, s0, s1, ptr(z), int(seed or 0), ptr(x), ptr(zo), int(bool(write_data)),
                                          L.i32p(info)), self._eng)
        if return_z:
            return x, info, (zo if z is None else z.copy())
        return x, info

    def simulated_nodes(self, x, site=0):
        """The states of simulate_lg by node, for an object built from labelled beliefs: {node label: [p]} for every node
        that has a family (the fixed root has none: its value is mu).  x: [sites, n_families, p]; site: which row."""
        if self._objs is None or self.node2family is None:
            raise ValueError("simulated_nodes needs labelled beliefs (an object built from CanonicalBelief objects)")
        x = np.asarray(x)
        skip = len(self.node2family) - x.shape[1]   # the root has no family unless it has a proper prior
        return {self.node2family[skip + f][0]: x[site, f].copy() for f in range(x.shape[1])}

    def _shift_gradient_from(self, d):
        e = getattr(self, "_lg_shift_edges", np.zeros(0, np.int32))
        nf = len(self._lg["cluster"])
        K = self._lg["length"].size // nf if nf else 1
        gam = self._lg["gamma"].reshape(-1)[e]
        return gam[None, :, None] * d["dshift"][:, e // K, :]

    def shift_gradient_lg(self, all_sites=False):
        """The derivative of the log-likelihood in every shift that is set: gamma_k * dshift[f] of edge_gradient_lg for the
        edges given to set_shifts_lg, in their order: [n, p], or [n_sites, n, p] when all_sites.  EXACT ONLY when the beliefs
        are calibrated on a clique tree under the current parameters and shifts, as edge_gradient_lg."""
        d = self.edge_gradient_lg(all_sites=True)
        s0 = 0 if all_sites else self.site
        if not all_sites and d["info"][s0]:
            raise np.linalg.LinAlgError(f"PosDefException: belief {d['info'][s0] - 1} is not positive definite")
        g = self._shift_gradient_from(d)
        return g if all_sites else g[s0].copy()

    def loglik_and_shift_gradient_lg(self, schedule_tree, all_sites=False):
        """Log-likelihood and its derivative in the shifts that are set, on a clique tree: the factors are filled again
        with the parameters of the last assignfactors_lg_ (so that shifts set since then are in), then the steps of
        loglik_and_edge_gradient_lg.  Returns (loglik, gradient [n, p]) of the current site, or arrays over the sites (NaN
        where a site failed) when all_sites."""
        if getattr(self, "_lg_last", None) is None:
            raise L.PgbpError(L.ERR_STATE, "loglik_and_shift_gradient_lg: no parameters yet (call assignfactors_lg_ first)")
        m, _keep = self._lg_last
        _check(self._lib.pgbp_lg_assignfactors(self._eng, C.byref(m)), self._eng)
        ll, d = self.loglik_and_edge_gradient_lg(schedule_tree, all_sites=True)
        g = self._shift_gradient_from(d)
        if all_sites:
            return ll, g
        if d["info"][self.site]:
            raise np.linalg.LinAlgError(f"PosDefException: belief {d['info'][self.site] - 1} is not positive definite")
        return float(ll[self.site]), g[self.site].copy()

    def shift_scan_lg(self, all_sites=False, min_info=1e-8, information=False):
        """pgbp_lg_shift_scan on the current beliefs: every edge scanned for a mean shift in one sweep over the node families.
        The log-likelihood is quadratic in a displacement d of a family's conditional mean; from the calibrated belief of the
        family's cluster the sweep forms the score g_w, the observed information H_f = j - j C j (C the covariance of the
        family's residual given the data) and returns the ML displacement H_f^-1 g_w and the gain 2 (ll(dhat) - ll(0)) =
        g_w' H_f^-1 g_w.  With shifts set it gives the INCREMENT to an edge's shift and the gain of a jump there while the
        other shifts stay where they are.  EXACT ONLY when the beliefs are calibrated (postorder and preorder) on a clique
        tree under the current parameters and shifts (not verified), as edge_gradient_lg.
        min_info: a trait whose pivot in H_f, given the kept traits before it (index order), is not above min_info * j_ii is
        not identified -- no tip below observes it, or the data leave the prior untouched -- and is dropped; the result is the
        ML displacement restricted to the kept traits.  (Rounding leaves such pivots at <= 2.6e-15 of j_ii on the test
        networks, identified ones are >= 2.8e-3 there; fit_shifts_lg uses 1e-10 on differences of scores.)
        Returns a dict, F = n_families, K = max_parents: jump [F, p] (NaN at a trait that is out of the family's child_mask or
        not identified, and for a root-prior family, which has no edge), lr [F] (0 when no trait is identified, NaN for a
        root-prior family), dof [F] (the number of kept traits), identified [F, p] (bool), edge_jump [F, K, p] = jump / gamma_k,
        the ML shift on parent edge k (NaN where there is no such edge or gamma_k = 0; its information is gamma_k^2 H, its lr
        the family's), info; with information=True also H [F, p, p] (H_f at the kept traits, NaN elsewhere) and se [F, p] =
        sqrt(diag(H_kept^-1)), the standard error of jump.  With a leading site axis when all_sites.  A site whose info is
        not 0 holds NaN; for the current site that raises."""
        p = self._lg_p
        nf = len(self._lg["cluster"])
        K = self._lg["length"].size // nf if nf else 1
        s0, s1 = (0, self.n_sites) if all_sites else (self.site, self.site + 1)
        n = s1 - s0
        jump = np.zeros((n, nf, p))
        lr = np.zeros((n, nf))
        ident = np.zeros((n, nf), np.uint64)
        H = np.zeros((n, nf, p, p)) if information else None
        info = np.zeros(n, dtype=np.int32)
        _check(self._lib.pgbp_lg_shift_scan(self._eng, s0, s1, float(min_info), L.f64p(jump), L.f64p(lr),
                                            ident.ctypes.data_as(C.POINTER(C.c_uint64)), L.f64p(H) if information else None,
                                            L.i32p(info)), self._eng)
        bits = ((ident[:, :, None] >> np.arange(p, dtype=np.uint64)[None, None, :]) & np.uint64(1)).astype(bool)
        gam = np.asarray(self._lg["gamma"], np.float64).reshape(nf, K)
        real = np.arange(K)[None, :] < np.asarray(self._lg["n_parents"]).reshape(nf, 1)
        inv = np.full((nf, K), np.nan)
        ok = real & (gam != 0.0)
        inv[ok] = 1.0 / gam[ok]
        d = dict(jump=jump, lr=lr, dof=bits.sum(axis=2).astype(np.int32), identified=bits,
                 edge_jump=jump[:, :, None, :] * inv[None, :, :, None], info=info)
        if information:
            se = np.full((n, nf, p), np.nan)
            flat_id, flat_H, flat_se = ident.reshape(-1), H.reshape(-1, p, p), se.reshape(-1, p)
            for mask in np.unique(flat_id):
                idx = [t for t in range(p) if (int(mask) >> t) & 1]
                if not idx:
                    continue
                sel = np.flatnonzero(flat_id == mask)
                cov = np.linalg.inv(flat_H[np.ix_(sel, idx, idx)])
                flat_se[np.ix_(sel, idx)] = np.sqrt(np.diagonal(cov, axis1=1, axis2=2))
            d["H"], d["se"] = H, se
        return d if all_sites else self._shift_scan_of_site(d, 0)

    @staticmethod
    def _shift_scan_of_site(d, s):
        if d["info"][s]:
            raise np.linalg.LinAlgError(f"PosDefException: belief {d['info'][s] - 1} is not positive definite")
        return dict({k: v[s].copy() for k, v in d.items() if k != "info"}, info=0)

    def loglik_and_shift_scan_lg(self, schedule_tree, all_sites=False, min_info=1e-8, information=False):
        """Log-likelihood and the scan of every edge for a mean shift, on a clique tree: the factors are filled again with the
        parameters of the last assignfactors_lg_ (so that shifts set since then are in), then the steps of
        loglik_and_edge_gradient_lg with the scan (shift_scan_lg) in place of the edge sweep.  Returns (loglik, scan dict): the
        current site's values, or arrays over the sites (info of a failed site is not 0 and its values are NaN) when
        all_sites."""
        if getattr(self, "_lg_last", None) is None:
            raise L.PgbpError(L.ERR_STATE, "loglik_and_shift_scan_lg: no parameters yet (call assignfactors_lg_ first)")
        m, _keep = self._lg_last
        _check(self._lib.pgbp_lg_assignfactors(self._eng, C.byref(m)), self._eng)
        self._ensure_schedule([schedule_tree])
        o = self._opts()
        pa = np.asarray(schedule_tree[-2]).reshape(-1)
        root = int(pa[0]) if pa.size else 0
        _check(self._lib.pgbp_enqueue_calibrate(self._eng, 1, 1, C.byref(o)), self._eng)
        _check(self._lib.pgbp_enqueue_integrate(self._eng, root), self._eng)
        scan = self.shift_scan_lg(all_sites=True, min_info=min_info, information=information)
        norm = np.zeros(self.n_sites)
        info = np.zeros(self.n_sites, dtype=np.int32)
        _check(self._lib.pgbp_fetch_loglik(self._eng, L.f64p(norm), L.i32p(info)), self._eng)
        scan["info"] = np.where(scan["info"] != 0, scan["info"], info)
        norm = np.where(scan["info"] != 0, np.nan, norm)
        if all_sites:
            return norm, scan
        return float(norm[self.site]), self._shift_scan_of_site(scan, self.site)

    def loo_lg(self, all_sites=False):
        """pgbp_lg_loo on the current beliefs: the leave-one-out predictive distribution of every tip that has data, given
        the data of all other tips, under the parameters of the last assignfactors_lg_ -- one sweep over the tip families.
        EXACT ONLY when the beliefs are calibrated (postorder and preorder) on a clique tree under those parameters (not
        verified); on a loopy cluster graph, at a converged calibration, it is the Bethe approximation.
        Returns a dict: families [n_tip] (indices into the family table given to lg_setup, the order of every other entry),
        mean [n_tip, p] and cov [n_tip, p, p] (NaN at unobserved traits), lpd [n_tip] (log predictive density of the tip's
        observed values), total (their sum in family order), info [n_tip] (0; 1: the other data do not determine the
        prediction; 1 + PosDefException.info of the cluster -- that tip's entries and total are NaN, nothing raises) and
        y [n_tip, p] (the tip's data row, for loo_zscores); with a leading site axis when all_sites."""
        p = self._lg_p
        nt = int(self._lib.pgbp_lg_loo_count(self._eng))
        if nt < 0:
            _check(self._lib.pgbp_lg_loo(self._eng, 0, 0, None, None, None, None, None), self._eng)
            raise L.PgbpError(L.ERR_STATE, "pgbp_lg_loo_count failed")
        fam = np.zeros(max(nt, 1), dtype=np.int32)
        _check(self._lib.pgbp_lg_loo_families(self._eng, L.i32p(fam)), self._eng)
        fam = fam[:nt]
        s0, s1 = (0, self.n_sites) if all_sites else (self.site, self.site + 1)
        n = s1 - s0
        mean = np.zeros((n, max(nt, 1), p))
        cov = np.zeros((n, max(nt, 1), p, p))
        lpd = np.zeros((n, max(nt, 1)))
        total = np.zeros(n)
        info = np.zeros((n, max(nt, 1)), dtype=np.int32)
        _check(self._lib.pgbp_lg_loo(self._eng, s0, s1, L.f64p(mean), L.f64p(cov), L.f64p(lpd), L.f64p(total), L.i32p(info)),
               self._eng)
        y = self._lg["data"][s0:s1][:, self._lg["data_row"][fam]]
        d = dict(families=fam, mean=mean[:, :nt], cov=cov[:, :nt].transpose(0, 1, 3, 2), lpd=lpd[:, :nt], total=total,
                 info=info[:, :nt], y=y)
        if all_sites:
            return d
        return {k: (v if k == "families" else (float(v[0]) if k == "total" else v[0].copy())) for k, v in d.items()}

    def loo_and_loglik_lg(self, schedule_tree, all_sites=False):
        """Log-likelihood and the leave-one-out predictions of every tip under the parameters of the last assignfactors_lg_
        on a clique tree: beliefs reset from the factors that call filled -> one calibrate (postorder + preorder of
        `schedule_tree`) -> integratebelief! at the tree's root cluster -> the sweep over the tip families (loo_lg), as
        loglik_and_gradient_lg does for the gradient.  Returns (loglik, loo dict): the current site's values, or arrays over
        the sites when all_sites (loglik of a site whose calibration failed is NaN)."""
        self._ensure_schedule([schedule_tree])
        o = self._opts()
        pa = np.asarray(schedule_tree[-2]).reshape(-1)
        root = int(pa[0]) if pa.size else 0
        _check(self._lib.pgbp_enqueue_calibrate(self._eng, 1, 1, C.byref(o)), self._eng)
        _check(self._lib.pgbp_enqueue_integrate(self._eng, root), self._eng)
        loo = self.loo_lg(all_sites=True)
        norm = np.zeros(self.n_sites)
        info = np.zeros(self.n_sites, dtype=np.int32)
        _check(self._lib.pgbp_fetch_loglik(self._eng, L.f64p(norm), L.i32p(info)), self._eng)
        norm = np.where(info != 0, np.nan, norm)
        if all_sites:
            return norm, loo
        s = self.site
        return float(norm[s]), {k: (v if k == "families" else (float(v[s]) if k == "total" else v[s].copy()))
                                for k, v in loo.items()}

    def impute_lg(self, all_sites=False):
        """pgbp_lg_impute on the current beliefs: the posterior mean and covariance of the MISSING values of every tip, given
        all the data (the tip's own observed traits included), under the parameters of the last assignfactors_lg_ -- one
        sweep over the tip families that miss a trait.  EXACT ONLY when the beliefs are calibrated (postorder and preorder)
        on a clique tree under those parameters (not verified); on a loopy cluster graph, at a converged calibration, it is
        the Bethe approximation.  A missing trait that a parent of the tip does not hold in scope (no tip below that parent
        observes it) is NOT predicted: NaN, predicted False -- the documented limit of the call.
        Returns a dict: families [n] (indices into the family table given to lg_setup, the order of every other entry),
        rows [n] (the data row of each tip), predicted [n, p] (bool, the same for every site), mean [n, p] and cov [n, p, p]
        (NaN outside predicted), info [n] (0; -1: nothing of this tip is predicted; 1: the tip's variance is not positive
        definite or its cluster's belief is still the constant 1; 1 + PosDefException.info of the cluster -- that tip's
        entries are NaN, nothing raises); mean, cov and info with a leading site axis when all_sites."""
        p = self._lg_p
        n = int(self._lib.pgbp_lg_impute_count(self._eng))
        if n < 0:
            _check(self._lib.pgbp_lg_impute(self._eng, 0, 0, None, None, None), self._eng)
            raise L.PgbpError(L.ERR_STATE, "pgbp_lg_impute_count failed")
        fam = np.zeros(max(n, 1), dtype=np.int32)
        pred = np.zeros(max(n, 1), dtype=np.uint64)
        _check(self._lib.pgbp_lg_impute_families(self._eng, L.i32p(fam), pred.ctypes.data_as(C.POINTER(C.c_uint64))), self._eng)
        fam, pred = fam[:n], pred[:n]
        s0, s1 = (0, self.n_sites) if all_sites else (self.site, self.site + 1)
        ns = s1 - s0
        mean = np.full((ns, max(n, 1), p), np.nan)
        cov = np.full((ns, max(n, 1), p, p), np.nan)
        info = np.zeros((ns, max(n, 1)), dtype=np.int32)
        _check(self._lib.pgbp_lg_impute(self._eng, s0, s1, L.f64p(mean), L.f64p(cov), L.i32p(info)), self._eng)
        predicted = ((pred[:, None] >> np.arange(p, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool).reshape(n, p)
        d = dict(families=fam, rows=self._lg["data_row"][fam], predicted=predicted, mean=mean[:, :n],
                 cov=cov[:, :n].transpose(0, 1, 3, 2), info=info[:, :n])
        if all_sites:
            return d
        return {k: (v[0].copy() if k in ("mean", "cov", "info") else v) for k, v in d.items()}

    def impute_and_loglik_lg(self, schedule_tree, all_sites=False):
        """Log-likelihood and the imputed values of every tip under the parameters of the last assignfactors_lg_ on a clique
        tree: beliefs reset from the factors that call filled -> one calibrate (postorder + preorder of `schedule_tree`) ->
        integratebelief! at the tree's root cluster -> the sweep over the listed tip families (impute_lg), as
        loo_and_loglik_lg does for the leave-one-out predictions.  Returns (loglik, impute dict): the current site's values,
        or arrays over the sites when all_sites (loglik of a site whose calibration failed is NaN)."""
        self._ensure_schedule([schedule_tree])
        o = self._opts()
        pa = np.asarray(schedule_tree[-2]).reshape(-1)
        root = int(pa[0]) if pa.size else 0
        _check(self._lib.pgbp_enqueue_calibrate(self._eng, 1, 1, C.byref(o)), self._eng)
        _check(self._lib.pgbp_enqueue_integrate(self._eng, root), self._eng)
        imp = self.impute_lg(all_sites=True)
        norm = np.zeros(self.n_sites)
        info = np.zeros(self.n_sites, dtype=np.int32)
        _check(self._lib.pgbp_fetch_loglik(self._eng, L.f64p(norm), L.i32p(info)), self._eng)
        norm = np.where(info != 0, np.nan, norm)
        if all_sites:
            return norm, imp
        s = self.site
        return float(norm[s]), {k: (v[s].copy() if k in ("mean", "cov", "info") else v) for k, v in imp.items()}

    def traffic_model(self):
        b = C.c_double()
        n = C.c_int64()
        _check(self._lib.pgbp_traffic_model(self._eng, C.byref(b), C.byref(n)), self._eng)
        return b.value, n.value


def loo_zscores(d):
    """Standardised leave-one-out residuals of the dict loo_lg returns: per tip z = L^-1 (y - mean) over its observed traits,
    cov = L L' (L lower triangular), so that z is standard normal under the model; NaN at unobserved traits and for a tip
    whose info is not 0.  Shape of d["mean"].  On the host."""
    mean, cov, y = np.asarray(d["mean"]), np.asarray(d["cov"]), np.asarray(d["y"])
    z = np.full(mean.shape, np.nan)
    for ix in np.ndindex(mean.shape[:-1]):
        o = np.isfinite(mean[ix])
        if o.any():
            z[ix][o] = np.linalg.solve(np.linalg.cholesky(cov[ix][np.ix_(o, o)]), (y[ix] - mean[ix])[o])
    return z


def imputed_data(d, data):
    """A copy of the data table [n_rows, p] (NaN where missing) with the entries the dict impute_lg returns predicts filled
    by their posterior mean (d["mean"] [n, p]: one site); every other missing entry stays NaN, and so does a tip whose info
    is not 0 -- but for info -2 (PGBP_INFO_NOT_OBSERVED: a tip of impute_sites_lg that is observed at this site under a
    per-site mask), whose entry of `data` is kept.  On the host."""
    out = np.array(data, dtype=np.float64, copy=True)
    mean, pred = np.asarray(d["mean"]), np.asarray(d["predicted"], bool)
    assert out.ndim == 2 and mean.ndim == 2, "one site: data [n_rows, p], d['mean'] [n, p]"
    info = np.asarray(d["info"]) if d.get("info") is not None else None
    for i, r in enumerate(np.asarray(d["rows"])):
        if info is not None and info.ndim == 1 and int(info[i]) == -2:
            continue   # (PGBP_INFO_NOT_OBSERVED: a tip observed at this site under a per-site mask, nothing to fill)
        out[int(r), pred[i]] = mean[i, pred[i]]
    return out


def split_missing_data(table, fill=0.0):
    """A univariate data table with NaN at its gaps, [n_sites, n_rows] (or [n_sites, n_rows, 1]), as (clean, mask): clean
    [n_sites, n_rows, 1] with `fill` at the gaps -- what lg_setup takes, which refuses values that are not finite -- and
    mask bool [n_sites, n_rows], True at the gaps -- what set_site_missing_lg takes.  The value at a gap is never used."""
    t = np.asarray(table, np.float64)
    if t.ndim == 3:
        assert t.shape[2] == 1, "per-site masks are univariate"
        t = t[:, :, 0]
    mask = np.isnan(t)
    return np.where(mask, float(fill), t)[:, :, None], mask


class _ResidualDict:
    """messageresidual: (label_to, label_from) -> MessageResidual (src/clustergraphbeliefs.jl:11-20).
    Keys may also be (index_to, index_from)."""

    def __init__(self, owner):
        self._o = owner

    def __getitem__(self, key):
        o = self._o
        to, frm = key
        if o.cdict is not None and to in o.cdict:
            to, frm = o.cdict[to], o.cdict[frm]
        d = o._msg_id(to, frm)
        return MessageResidual(o, d, int(o._dims[o.nclusters + d // 2]))

    def __len__(self):
        return 2 * self._o.nsepsets
