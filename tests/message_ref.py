"""Tests only: a numpy.longdouble restatement of ONE message of the reference (src/beliefupdates.jl), the input
generators that place a message at the shape limits of the wave-per-task kernels, and the case lists shared by
tests/test_message_ref_cpu.py (no GPU: the reference pinned to oracle/beliefupdates.py and to the plain-C engine) and
tests/test_gpu_message_shapes.py (the device against the same reference).

numpy only, no library factorisation in the reference: the Cholesky below is written out row by row (the house style of
the inverse in tests/test_gpu_moments.py).  Every generated input is well conditioned by construction; nothing here is
about conditioning.
"""
import zlib
from collections import namedtuple

import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
PI_LD = 4 * np.arctan(LD(1))
LOG2PI_LD = np.log(2 * PI_LD)

# the shape limits of the kernels (csrc/pgbp_internal.hpp, include/pgbp.h), restated for the case lists
SMALL_I, SMALL_K, GENERIC_MAX, LDS_MAX, REC_BYTE_MAX, MAX_DIM = 8, 8, 64, 128, 254, 384
BODIES = ("small", "inlds", "biglds", "bigws")


def body_of(mf, s, mt):
    """Which message body pgbp_propagate runs for a shape (bp_level_generic: small / in-LDS; bp_level_big: LDS / workspace)."""
    if mf > LDS_MAX:
        return "bigws"
    if mf > GENERIC_MAX or mt > REC_BYTE_MAX:
        return "biglds"
    return "small" if (mf - s <= SMALL_I and s <= SMALL_K) else "inlds"


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------

def chol_upper_rows(A, dtype=LD):
    """PDMat(Symmetric(A)) (src/beliefupdates.jl:68): A = U'U reading the UPPER triangle of A only, one row of U at a time.
    Returns (U, info, pivot): info the 1-based index of the first pivot that is not > 0 (0: none), pivot its value."""
    A = np.asarray(A, dtype=dtype)
    n = A.shape[0]
    U = np.zeros((n, n), dtype=dtype)
    for j in range(n):
        d = A[j, j] - (U[:j, j] * U[:j, j]).sum(dtype=dtype)
        if not d > 0:
            return U, j + 1, d
        U[j, j] = np.sqrt(d)
        if j + 1 < n:
            U[j, j + 1:] = (A[j, j + 1:] - U[:j, j] @ U[:j, j + 1:]) / U[j, j]
    return U, 0, dtype(0)


def _solve_ut(U, B):
    """X with U'X = B (U upper triangular), row by row."""
    n = U.shape[0]
    X = np.zeros(B.shape, dtype=LD)
    for b in range(n):
        X[b] = (B[b] - U[:b, b] @ X[:b]) / U[b, b]
    return X


def _solve_u(U, B):
    n = U.shape[0]
    X = np.zeros(B.shape, dtype=LD)
    for b in range(n - 1, -1, -1):
        X[b] = (B[b] - U[b, b + 1:] @ X[b + 1:]) / U[b, b]
    return X


def marginalize_ld(J, h, g, keep_idx):
    """src/beliefupdates.jl:55-83 in longdouble.  Returns (J_msg, h_msg, g_msg, info, exit): exit 1 = nothing to integrate
    (:56), 2 = the all-zero block (:62-66, decided on the float64 inputs), 0 = the Cholesky path; info != 0: no message."""
    J64, h64 = np.asarray(J, dtype=np.float64), np.asarray(h, dtype=np.float64)
    keep = np.asarray(keep_idx, dtype=np.int64).reshape(-1)
    mask = np.ones(h64.shape[0], dtype=bool)
    mask[keep] = False
    integ = np.nonzero(mask)[0]                  # :52 setdiff, ascending
    Jl, hl, gl = J64.astype(LD), h64.astype(LD), LD(g)
    if integ.size == 0:                          # :56
        return Jl, hl, gl, 0, 1
    Ji, Jk, Jki = J64[np.ix_(integ, integ)], Jl[np.ix_(keep, keep)], J64[np.ix_(keep, integ)]
    hi, hk = h64[integ], hl[keep]
    if np.all(np.abs(Ji) <= EPS) and np.all(np.abs(hi) <= EPS) and np.all(np.abs(Jki) <= EPS):   # :62-66
        return Jk, hk, gl, 0, 2
    U, info, _ = chol_upper_rows(Ji)             # :68
    if info:
        return None, None, None, info, 0
    Z = _solve_ut(U, Jki.T.astype(LD))           # :77  Jki Ji^-1 Jki' = Z'Z
    Jm = Jk - Z.T @ Z
    mu = _solve_u(U, _solve_ut(U, hi.astype(LD)))   # :78
    hm = hk - Jki.astype(LD) @ mu                # :79
    logdet = 2 * np.log(np.diag(U)).sum(dtype=LD)
    gm = gl + (integ.size * LOG2PI_LD - logdet + hi.astype(LD) @ mu) / 2   # :81
    return Jm, hm, gm, 0, 0


def propagate_ld(sender, sepset, receiver, keep_idx, up_idx):
    """marginalize (:55-83), divide! (:579-587) and mult! (:483-488) of one message, in longdouble.  sender / sepset /
    receiver: (J, h, g).  Returns (new sepset, new receiver, (dJ, dh), info, exit); on info != 0 nothing is changed (the
    inputs come back, the residual is None)."""
    Jm, hm, gm, info, ex = marginalize_ld(*sender, keep_idx)
    Js, hs, gs = np.asarray(sepset[0], dtype=LD), np.asarray(sepset[1], dtype=LD), LD(sepset[2])
    Jt, ht, gt = np.array(receiver[0], dtype=LD), np.array(receiver[1], dtype=LD), LD(receiver[2])
    if info:
        return (Js, hs, gs), (Jt, ht, gt), None, info, ex
    dJ, dh, dg = Jm - Js, hm - hs, gm - gs       # divide!
    up = np.asarray(up_idx, dtype=np.int64).reshape(-1)
    Jt[np.ix_(up, up)] += dJ                      # mult!
    ht[up] += dh
    gt = gt + dg
    return (Jm, hm, gm), (Jt, ht, gt), (dJ, dh), 0, ex


def integrate_ld(J, h, g):
    """src/beliefupdates.jl:187-200 in longdouble: (mu, norm, info)."""
    J64, h64 = np.asarray(J, dtype=np.float64), np.asarray(h, dtype=np.float64)
    if not h64.any() and not J64.any():          # :189-191
        return np.full(h64.shape, np.inf, dtype=LD), LD(g), 0
    U, info, _ = chol_upper_rows(J64)
    if info:
        return None, None, info
    hl = h64.astype(LD)
    mu = _solve_u(U, _solve_ut(U, hl))
    logdet = 2 * np.log(np.diag(U)).sum(dtype=LD)
    return mu, LD(g) + (h64.shape[0] * LOG2PI_LD - logdet + (hl * mu).sum(dtype=LD)) / 2, 0


def residnorm_flag_ld(dJ, dh, atol=1e-5):
    """iscalibrated_residnorm! (src/beliefs.jl:994-997), max norm, on a longdouble residual; an empty residual is calibrated."""
    if dh.size == 0:
        return True
    return bool(np.abs(dh).max() / np.sqrt(LD(dh.size)) <= atol and np.abs(dJ).max() / np.sqrt(LD(dJ.size)) <= atol)


# ---------------------------------------------------------------------------------------------------------------------
# input generators
# ---------------------------------------------------------------------------------------------------------------------

def spd(rng, n, lo=1.0, hi=10.0):
    """Q diag(lambda) Q' with lambda spread over [lo, hi] (both ends attained), Q a product of Householder reflectors: every
    principal block has its eigenvalues in [lo, hi] (interlacing), so its condition number is at most hi / lo."""
    if n == 0:
        return np.zeros((0, 0))
    lam = rng.uniform(lo, hi, n)
    lam[0] = lo
    lam[-1] = hi
    A = np.diag(rng.permutation(lam))
    for _ in range(min(n, 6)):
        v = rng.standard_normal(n)
        v /= np.sqrt(v @ v)
        A = A - 2.0 * np.outer(v, v @ A)
        A = A - 2.0 * np.outer(A @ v, v)
    return (A + A.T) / 2


def ldl_failure(rng, n, k, kind):
    """J = L D L' with unit lower-triangular L whose k-th pivot (1-based) is the first that is not positive.
    kind "sign": |L_ij| <= 0.25, D in [1, 10] except D_k = -1: the leading k - 1 minors clearly positive, the k-th clearly
    negative.  kind "zero": L from {0, +-1/2, +-1/4}, D from {1, 4} except D_k = 0: every entry of J, every Schur complement
    and every Cholesky entry (sqrt D in {1, 2}) is a multiple of 1/16 below 2^12 for n <= 384 -- exact in float64 in any
    order of operations, so pivot k is exactly 0.0."""
    L = np.eye(n)
    if kind == "sign":
        L += np.tril(rng.uniform(-0.25, 0.25, (n, n)), -1)
        D = rng.uniform(1.0, 10.0, n)
        D[k - 1] = -1.0
    else:
        L += np.tril(rng.choice([0.0, 0.0, 0.5, -0.5, 0.25, -0.25], (n, n)), -1)
        D = rng.choice([1.0, 4.0], n)
        D[k - 1] = 0.0
    J = (L * D) @ L.T
    return (J + J.T) / 2


PATTERNS = ("lead", "trail", "alt", "rand")


def index_pattern(kind, n, s, rng):
    """s of n positions, strictly increasing: a leading block, a trailing block, every other variable (kept while they fit,
    else every other variable is the one left out), a random subset."""
    if kind == "lead":
        idx = np.arange(s)
    elif kind == "trail":
        idx = np.arange(n - s, n)
    elif kind == "alt":
        if 2 * s - 1 <= n:
            idx = np.arange(0, 2 * s, 2)
        else:
            out = np.arange(1, 2 * (n - s), 2)
            idx = np.setdiff1d(np.arange(n), out)
    else:
        idx = np.sort(rng.choice(n, s, replace=False))
    idx = idx.astype(np.int32)
    assert idx.size == s and (s == 0 or (idx[0] >= 0 and idx[-1] < n)) and np.all(np.diff(idx) > 0)
    return idx


# ---------------------------------------------------------------------------------------------------------------------
# cases.  One engine per case: two clusters (sender, receiver; `flip` swaps their indices, so both message directions
# occur) and one sepset, two sites with different numbers.
# ---------------------------------------------------------------------------------------------------------------------

Case = namedtuple("Case", "name mf s mt keep_kind up_kind sep_kind flip fail")
# sep_kind: "zero" (the sepset starts as the constant 1), "below" (half the marginal: SPD below it), "near" (the marginal
# to 1e-9 relative: the residual passes iscalibrated_residnorm by a factor 1e3 and more).
# fail: None | (site, k, kind) a pivot-placed failure in that site | ("exit2", c) J_I = c I, h_I = 0, J_KI = 0 in site 0.


def _mt_for(s, i, up_kind):
    mt = s + (0, 1, 5)[i % 3]
    if up_kind == "alt":
        mt = max(mt, 2 * s - 1)
    return max(1, min(mt, REC_BYTE_MAX if s <= REC_BYTE_MAX else MAX_DIM))


def shape_cases():
    """(a): the shapes on both sides of every limit."""
    shapes = []
    for ni, s in [(1, 1), (8, 8), (8, 1), (1, 8), (0, 8), (8, 0), (9, 8), (8, 9), (9, 9)]:
        shapes.append((ni + s, s, None))
    for mf in (17, 33, 63, 64):
        shapes += [(mf, s, None) for s in (0, 1, mf // 2, mf - 1, mf)]
    for mf in (65, 96, 127, 128):
        shapes += [(mf, s, None) for s in (1, 64, mf - 1)]
    for mf in (129, 192, 384):
        shapes += [(mf, s, None) for s in (1, 128, mf - 1)]
    shapes += [(4, 2, mt) for mt in (254, 255, 384)]
    out = []
    for i, (mf, s, mt) in enumerate(shapes):
        keep_kind, up_kind = PATTERNS[i % 4], PATTERNS[(i // 4 + i) % 4]
        if mt is None:
            mt = _mt_for(s, i, up_kind)
            if body_of(mf, s, 1) == "bigws" and s > REC_BYTE_MAX:
                mt = min(MAX_DIM, s + i % 2)
        sep_kind = ("zero", "below", "near")[i % 3]
        out.append(Case(f"a-{mf}-{s}-{mt}-{keep_kind}-{up_kind}-{sep_kind}", mf, s, mt, keep_kind, up_kind, sep_kind,
                        bool(i % 2), None))
    for body in BODIES:   # every index pattern at least once per body, on the sender side and on the receiver side
        mine = [c for c in out if body_of(c.mf, c.s, c.mt) == body]
        assert {c.keep_kind for c in mine} == set(PATTERNS) and {c.up_kind for c in mine} == set(PATTERNS), body
    return out


_BODY_SHAPE = {"small": (10, 2, 4, "rand"), "inlds": (64, 1, 3, "lead"), "biglds": (128, 1, 2, "trail"),
               "bigws": (192, 2, 5, "alt")}


def pivots_for(ni):
    ks = {1, 2, (ni + 1) // 2, ni} | {k for k in (16, 17, 64, 65) if k <= ni}
    return sorted(k for k in ks if 1 <= k <= ni)


def exit2_cases():
    """(b): J_I = c I, h_I = 0, J_KI = 0 with c = eps (the all-zero exit) and c = 2 eps (no exit), once per body."""
    out = []
    for body in BODIES:
        mf, s, mt, keep_kind = _BODY_SHAPE[body]
        for c in (EPS, 2 * EPS):
            out.append(Case(f"b-{body}-{c / EPS:.0f}eps", mf, s, mt, keep_kind, "rand", "below", body in ("inlds", "bigws"),
                            ("exit2", c)))
    return out


def failure_cases():
    """(c): a failure placed at pivot k of one site (alternating), the other site good, per body and per generator."""
    out = []
    for body in BODIES:
        mf, s, mt, keep_kind = _BODY_SHAPE[body]
        for kind in ("sign", "zero"):
            for j, k in enumerate(pivots_for(mf - s)):
                out.append(Case(f"c-{body}-{kind}-k{k}", mf, s, mt, keep_kind, "rand", "below", bool(j % 2), (j % 2, k, kind)))
    return out


def all_message_cases():
    return shape_cases() + exit2_cases() + failure_cases()


INTEGRATE_DIMS = (1, 2, 16, 17, 64, 128, 129, 384)
INTEGRATE_FAIL_DIMS = (16, 17, 128, 129)


def integrate_failure_cases():
    return [(m, k, kind, j % 2) for m in INTEGRATE_FAIL_DIMS for kind in ("sign", "zero") for j, k in enumerate(pivots_for(m))]


def _rng_of(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _belief(rng, n, J=None):
    return (spd(rng, n) if J is None else J, rng.standard_normal(n), float(rng.standard_normal()))


Built = namedtuple("Built", "case keep up senders sepsets receivers dims sepcl scope_off scope_idx packed i_from i_to")


def build_case(case, n_sites=2):
    """The float64 inputs of a case: per site (J, h, g) of sender, sepset and receiver, the index maps, and the engine
    description with its packed beliefs [n_sites, packed_size].  Sites beyond the first two are drawn after them
    (_site_inputs), so the first two are the same bytes whatever n_sites is."""
    rng = _rng_of(case.name)
    mf, s, mt = case.mf, case.s, case.mt
    keep = index_pattern(case.keep_kind, mf, s, rng)
    up = index_pattern(case.up_kind, mt, s, rng)
    integ = np.setdiff1d(np.arange(mf), keep)
    senders, sepsets, receivers = [], [], []
    for site in range(2):
        snd = _belief(rng, mf)
        if integ.size:
            w = np.linalg.eigvalsh(snd[0][np.ix_(integ, integ)])
            assert w[0] > 0 and w[-1] / w[0] <= 10.0 * (1 + 1e-12), case   # condition number of J_I by construction
        f = case.fail
        if f is not None and f[0] == "exit2" and site == 0:
            J = snd[0]
            J[np.ix_(integ, integ)] = f[1] * np.eye(integ.size)
            J[np.ix_(keep, integ)] = 0.0
            J[np.ix_(integ, keep)] = 0.0
            snd[1][integ] = 0.0
        elif f is not None and f[0] == site:
            J = snd[0]
            J[np.ix_(integ, integ)] = ldl_failure(rng, integ.size, f[1], f[2])
        rcv = _belief(rng, mt)
        Jm, hm, gm, info, _ = marginalize_ld(*snd, keep)
        if case.sep_kind == "zero" or info:
            sep = (np.zeros((s, s)), np.zeros(s), 0.0)
        else:
            q = 0.5 if case.sep_kind == "below" else 1.0 - 1e-9
            sep = ((q * Jm).astype(np.float64), (q * hm).astype(np.float64) + (0.0 if q > 0.9 else 0.1), float(rng.standard_normal()))
        senders.append(snd)
        sepsets.append(sep)
        receivers.append(rcv)
    for site in range(2, n_sites):
        snd, sep, rcv = _site_inputs(case, rng, site, keep, integ, n_sites)
        senders.append(snd)
        sepsets.append(sep)
        receivers.append(rcv)
    i_from, i_to = (1, 0) if case.flip else (0, 1)
    dims = np.zeros(3, np.int32)
    dims[i_from], dims[i_to], dims[2] = mf, mt, s
    sides = [None, None]
    sides[i_from], sides[i_to] = keep, up
    scope_off = np.array([0, s, 2 * s], np.int64)
    scope_idx = np.concatenate(sides).astype(np.int32)
    packed = []
    for site in range(n_sites):
        recs = [None, None, sepsets[site]]
        recs[i_from], recs[i_to] = senders[site], receivers[site]
        packed.append(np.concatenate([pack_record(*r) for r in recs]))
    return Built(case, keep, up, senders, sepsets, receivers, dims, np.array([0, 1], np.int32), scope_off, scope_idx,
                 np.stack(packed), i_from, i_to)


def pack_record(J, h, g):
    """The packed record of include/pgbp.h: J column-major, h, g."""
    return np.concatenate([np.asarray(J, np.float64).reshape(-1, order="F"), np.asarray(h, np.float64), [float(g)]])


def unpack_record(rec, m):
    rec = np.asarray(rec)
    return rec[:m * m].reshape(m, m, order="F"), rec[m * m:m * m + m], rec[m * m + m]


def record_offsets(dims):
    d = np.asarray(dims, np.int64)
    return np.concatenate([[0], np.cumsum(d * d + d + 1)])


def records_of(built, packed_site):
    """(sender, sepset, receiver) records (J, h, g) of one site's packed beliefs."""
    off = record_offsets(built.dims)
    rec = lambda i: unpack_record(packed_site[off[i]:off[i + 1]], int(built.dims[i]))
    return rec(built.i_from), rec(2), rec(built.i_to)


def reference_of(built, site, packed_site=None):
    """propagate_ld on one site of a built case (packed_site: on these float64 beliefs instead of the case's own)."""
    snd, sep, rcv = records_of(built, built.packed[site] if packed_site is None else packed_site)
    return propagate_ld(snd, sep, rcv, built.keep, built.up)


def record_error(got, want):
    """(max |got - want| over J, h, g of a record; max(1, |want|_inf)): the project's per-record measure."""
    err, scale = 0.0, 1.0
    for a, b in zip(got, want):
        a, b = np.asarray(a, dtype=LD).reshape(-1), np.asarray(b, dtype=LD).reshape(-1)
        if b.size:
            err = max(err, float(np.abs(a - b).max()))
            scale = max(scale, float(np.abs(b).max()))
    return err, scale


def c_engine_message(built, site, packed_site=None):
    """The plain-C engine (oracle/cengine.py) on one site of a built case: (sepset, receiver, (dJ, dh), sender, info, flag)."""
    from oracle import cengine
    ce = cengine.Engine(built.dims, built.sepcl, built.scope_off, built.scope_idx,
                        built.packed[site] if packed_site is None else packed_site)
    info = ce.propagate(built.i_to, 0, built.i_from)
    out = ce.packed()
    off = record_offsets(built.dims)
    rec = lambda i: unpack_record(out[off[i]:off[i + 1]], int(built.dims[i]))
    res, flags = ce.residuals()
    s = built.case.s
    d = 1 if built.i_to == 1 else 0        # message id 2k + dir: dir 1 = received by the sepset's second cluster
    r = res[d * (s * s + s):(d + 1) * (s * s + s)]
    return rec(2), rec(built.i_to), (r[:s * s].reshape(s, s, order="F"), r[s * s:]), rec(built.i_from), info, bool(flags[d])


def c_engine_errors(built, site, ref=None, packed_site=None):
    """Errors of the float64 C engine against the longdouble reference on one site: {"sepset", "receiver", "residual"} ->
    (error, scale).  The measuring stick of the device tests."""
    sep, rcv, res, _, info, _ = c_engine_message(built, site, packed_site)
    new_sep, new_rcv, resid, rinfo, _ = ref if ref is not None else reference_of(built, site, packed_site)
    assert info == rinfo == 0
    return {"sepset": record_error(sep, new_sep), "receiver": record_error(rcv, new_rcv),
            "residual": record_error(res, resid)}


def integrate_inputs(m, fail=None):
    """Two sites of an m-variable belief for pgbp_integrate (beside a one-variable neighbour, so that the engine is an
    ordinary two-cluster graph).  fail: None | (site, k, kind)."""
    rng = _rng_of(f"int-{m}-{fail}")
    beliefs = []
    for site in range(2):
        J = ldl_failure(rng, m, fail[1], fail[2]) if fail is not None and fail[0] == site else None
        beliefs.append(_belief(rng, m, J))
    dims = np.array([m, 1, 1], np.int32)
    scope_off = np.array([0, 1, 2], np.int64)
    scope_idx = np.array([m - 1, 0], np.int32)
    one = (np.ones((1, 1)), np.zeros(1), 0.0)
    packed = np.stack([np.concatenate([pack_record(*b), pack_record(*one), pack_record(*one)]) for b in beliefs])
    return beliefs, dims, np.array([0, 1], np.int32), scope_off, scope_idx, packed


def c_engine_integrate(dims, sepcl, scope_off, scope_idx, packed_site):
    """(mu, norm, info) of the plain-C engine's integratebelief on belief 0."""
    import ctypes as C
    from oracle import cengine
    ce = cengine.Engine(dims, sepcl, scope_off, scope_idx, packed_site)
    m = int(dims[0])
    mu = np.zeros(max(1, m))
    norm = C.c_double()
    info = cengine.lib().orc_integrate(ce.h, 0, mu.ctypes.data_as(C.POINTER(C.c_double)), C.byref(norm))
    return mu[:m], norm.value, int(info)


# ---------------------------------------------------------------------------------------------------------------------
# the tiny shapes of the thread-per-site kernels (bp_level_uni, bp_level_uni1, bp_chunk_uni1: every belief <= 2 variables,
# lanes = sites), many sites.  Shared by tests/test_uni_cases_cpu.py and tests/test_gpu_uni_message_shapes.py.
# ---------------------------------------------------------------------------------------------------------------------

UNI_SITES = (8, 64, 65)      # thread-per-site in the plain layout / the smallest site-minor batch / a padded site-minor row
UNI_MAX_SITES = max(UNI_SITES)
SEP_KINDS = ("zero", "below", "near")


def _maps(n, s):
    """every strictly increasing map of s positions into n (n <= 2) by its pattern name"""
    return ("lead", "trail") if (s == 1 and n == 2) else ("lead",)


def uni_shape_cases():
    """Every (mf, s, mt) with mf, mt in {0, 1, 2} and s <= min(mf, mt), every strictly increasing keep map and up map, all
    three sepset kinds, both directions: 19 shapes-with-maps x 3 x 2 = 114 cases."""
    out = []
    for mf in range(3):
        for mt in range(3):
            for s in range(min(mf, mt) + 1):
                for kk in _maps(mf, s):
                    for uk in _maps(mt, s):
                        for sep_kind in SEP_KINDS:
                            for flip in (False, True):
                                out.append(Case(f"u-{mf}-{s}-{mt}-{kk}-{uk}-{sep_kind}-{int(flip)}", mf, s, mt, kk, uk, sep_kind,
                                                flip, None))
    return out


# the sites that carry a placed event: not lane 0 of their wavefront, and site 64 (the one site of the padded row of a
# 65-site batch)
UNI_EVENT_SITES = {8: (5,), 64: (37,), 65: (37, 64)}
_UNI_EXIT_SHAPES = ((1, 1), (1, 0), (2, 0))        # (ni, s)


def uni_exit2_cases():
    """The all-zero exit at c = eps and no exit at c = 2 eps, for (ni, s) = (1, 1), (1, 0), (2, 0); placed in site 0 (as
    exit2_cases) and in the event sites."""
    return [Case(f"ub-{ni}-{s}-{c / EPS:.0f}eps", ni + s, s, 2, "trail" if s else "lead", "trail" if s else "lead", "below",
                 bool(ni % 2), ("exit2", c))
            for ni, s in _UNI_EXIT_SHAPES for c in (EPS, 2 * EPS)]


def uni_failure_cases():
    """A failure at pivot 1 (ni = 1, 2) and at pivot 2 (ni = 2) of the event sites, both generators, s = 0 and s = 1 where
    the shape allows (mf <= 2)."""
    out = []
    for ni, s in ((1, 0), (1, 1), (2, 0)):
        for k in range(1, ni + 1):
            for kind in ("sign", "zero"):
                out.append(Case(f"uc-{ni}-{s}-k{k}-{kind}", ni + s, s, 2, "lead", "trail" if s else "lead", "below", bool(k % 2),
                                ("sites", k, kind)))
    return out


def _site_inputs(case, rng, site, keep, integ, n_sites):
    """(sender, sepset, receiver) of one site beyond the first two of build_case: the same construction, with the
    eigenvalue range of every matrix drawn per site (a 1 x 1 spd() is always 10)."""
    mf, s, mt = case.mf, case.s, case.mt
    lo = rng.uniform(0.5, 2.0)
    hi = lo * rng.uniform(2.0, 10.0)
    snd = (spd(rng, mf, lo, hi), rng.standard_normal(mf), float(rng.standard_normal()))
    f = case.fail
    events = UNI_EVENT_SITES.get(n_sites, ())
    if f is not None and site in events:
        J = snd[0]
        if f[0] == "exit2":
            J[np.ix_(integ, integ)] = f[1] * np.eye(integ.size)
            J[np.ix_(keep, integ)] = 0.0
            J[np.ix_(integ, keep)] = 0.0
            snd[1][integ] = 0.0
        elif f[0] == "sites":
            J[np.ix_(integ, integ)] = ldl_failure(rng, integ.size, f[1], f[2])
    rcv = (spd(rng, mt, lo, hi), rng.standard_normal(mt), float(rng.standard_normal()))
    Jm, hm, gm, info, _ = marginalize_ld(*snd, keep)
    if case.sep_kind == "zero" or info:
        sep = (np.zeros((s, s)), np.zeros(s), 0.0)
    else:
        q = 0.5 if case.sep_kind == "below" else 1.0 - 1e-9
        sep = ((q * Jm).astype(np.float64), (q * hm).astype(np.float64) + (0.0 if q > 0.9 else 0.1), float(rng.standard_normal()))
    return snd, sep, rcv


Msg = namedtuple("Msg", "i_from i_to k keep up")     # k: the sepset's number (belief index n_clusters + k)
UniBuilt = namedtuple("UniBuilt", "case kind n_sites dims sepcl scope_off scope_idx packed msgs pa ch nc fail_sites")
UNI_KINDS = ("pair", "chain2", "chain1")
# pair:   sender -(s)- receiver                                   rooted at the receiver: one message
# chain2: sender -(s)- receiver -(2)- extra(2)                    (mt = 2); for mt < 2 one more link carries the 2-variable
#         sender -(s)- receiver -(mt)- extra(2) -(2)- extra(2)    sepset.  The engine's largest sepset is 2 whatever s is.
# chain1: sender -(s)- receiver -(min(1, mt))- extra(2)           s <= 1: every sepset <= 1 and two levels (a chunk)
# chains are rooted at their last cluster: the postorder sends sender -> receiver first, then the message OUT OF the receiver.


def build_uni(case, kind="pair", n_sites=2):
    """A case on an engine of n_sites sites (sites 0 and 1: build_case's bytes; further sites drawn after them)."""
    b = build_case(case, n_sites)
    fail_sites = tuple(x for x in UNI_EVENT_SITES.get(n_sites, ()) if case.fail is not None and case.fail[0] == "sites")
    first = Msg(b.i_from, b.i_to, 0, b.keep, b.up)
    if kind == "pair":
        return UniBuilt(case, kind, n_sites, b.dims, b.sepcl, b.scope_off, b.scope_idx, b.packed, [first],
                        np.array([b.i_to], np.int32), np.array([b.i_from], np.int32), 2, fail_sites)
    rng = _rng_of(case.name + "-" + kind)
    mt = case.mt
    if kind == "chain2":
        links = [(2, 2)] if mt == 2 else [(mt, 2), (2, 2)]      # (sepset dimension, next cluster's dimension)
    else:
        assert case.s <= 1
        links = [(min(1, mt), 2)]
    nc = 2 + len(links)
    cdims = [int(b.dims[0]), int(b.dims[1])] + [d for _, d in links]
    sdims = [case.s] + [s2 for s2, _ in links]
    sepcl = [0, 1]
    sides = [b.scope_idx[b.scope_off[0]:b.scope_off[1]], b.scope_idx[b.scope_off[1]:b.scope_off[2]]]
    msgs = [first]
    prev = b.i_to
    for j, (s2, d) in enumerate(links):
        nxt = 2 + j
        dp = cdims[prev]
        kp = np.arange(s2, dtype=np.int32)                                    # every variable of a receiver of mt < 2
        un = np.arange(d - s2, d, dtype=np.int32)                             # the trailing variables of the next cluster
        if (j + int(case.flip)) % 2:
            sepcl += [nxt, prev]
            sides += [un, kp]
        else:
            sepcl += [prev, nxt]
            sides += [kp, un]
        assert s2 <= dp
        msgs.append(Msg(prev, nxt, 1 + j, kp, un))
        prev = nxt
    scope_off = np.concatenate([[0], np.cumsum([len(x) for x in sides])]).astype(np.int64)
    scope_idx = np.concatenate(sides).astype(np.int32)
    dims = np.array(cdims + sdims, np.int32)
    off0 = record_offsets(b.dims)
    packed = []
    for site in range(n_sites):
        recs = [b.packed[site][off0[0]:off0[1]], b.packed[site][off0[1]:off0[2]]]
        lo = rng.uniform(0.5, 2.0)
        for _, d in links:
            recs.append(pack_record(spd(rng, d, lo, 8.0 * lo), rng.standard_normal(d), float(rng.standard_normal())))
        recs.append(b.packed[site][off0[2]:off0[3]])
        for s2, _ in links:
            if case.sep_kind == "zero":
                recs.append(np.zeros(s2 * s2 + s2 + 1))
            else:
                recs.append(pack_record(spd(rng, s2, 0.1 * lo, 0.4 * lo), 0.1 * rng.standard_normal(s2), float(rng.standard_normal())))
        packed.append(np.concatenate(recs))
    pa = np.array([m.i_to for m in reversed(msgs)], np.int32)      # preorder from the root = the last cluster
    ch = np.array([m.i_from for m in reversed(msgs)], np.int32)
    return UniBuilt(case, kind, n_sites, dims, np.array(sepcl, np.int32), scope_off, scope_idx, np.stack(packed), msgs, pa, ch,
                    nc, fail_sites)


def uni_records(ub, packed_site):
    """every belief record (J, h, g) of one site's packed beliefs"""
    off = record_offsets(ub.dims)
    return [unpack_record(packed_site[off[i]:off[i + 1]], int(ub.dims[i])) for i in range(len(ub.dims))]


def uni_reference(ub, packed_site):
    """The postorder of ub in longdouble on one site's float64 beliefs: per message (new sepset, new receiver, residual,
    info, exit) or None for a message that is not sent (its sender received no message because of a failure upstream).
    The sender of a later message is the previous receiver ROUNDED to float64: what an engine holds."""
    recs = uni_records(ub, packed_site)
    out, dead = [], set()
    for m in ub.msgs:
        if m.i_from in dead:
            dead.add(m.i_to)
            out.append(None)
            continue
        r = propagate_ld(recs[m.i_from], recs[ub.nc + m.k], recs[m.i_to], m.keep, m.up)
        out.append(r)
        if r[3]:
            dead.add(m.i_to)
            continue
        recs[ub.nc + m.k] = tuple(np.asarray(x, dtype=LD).astype(np.float64) for x in r[0])
        recs[m.i_to] = tuple(np.asarray(x, dtype=LD).astype(np.float64) for x in r[1])
    return out


def uni_c_engine(ub, packed_site):
    """The plain-C engine on the same postorder of one site: (packed beliefs, residual records, flags, infos)."""
    from oracle import cengine
    ce = cengine.Engine(ub.dims, ub.sepcl, ub.scope_off, ub.scope_idx, packed_site)
    infos, dead = [], set()
    for m in ub.msgs:
        if m.i_from in dead:
            dead.add(m.i_to)
            infos.append(None)
            continue
        infos.append(ce.propagate(m.i_to, m.k, m.i_from))
        if infos[-1]:
            dead.add(m.i_to)
    res, flags = ce.residuals()
    return ce.packed(), res, flags, infos


def residual_of(ub, m, res_site):
    """(dJ, dh) of message m in one site's residual records, and the message's id (2 k + direction)"""
    sd = np.repeat(ub.dims[ub.nc:].astype(np.int64), 2)
    roff = np.concatenate([[0], np.cumsum(sd * sd + sd)])
    d = 2 * m.k + (1 if ub.sepcl[2 * m.k + 1] == m.i_to else 0)
    s = int(ub.dims[ub.nc + m.k])
    r = res_site[roff[d]:roff[d + 1]]
    return (r[:s * s].reshape(s, s, order="F"), r[s * s:]), d


def uni_integrate_inputs(m, n_sites):
    """n_sites beliefs of m <= 2 variables for pgbp_integrate beside a one-variable neighbour (integrate_inputs' engine);
    the event sites hold a failure at pivot m ("sign")."""
    rng = _rng_of(f"uint-{m}-{n_sites}")
    beliefs = []
    for site in range(n_sites):
        lo = rng.uniform(0.5, 2.0)
        J = ldl_failure(rng, m, m, "sign") if site in UNI_EVENT_SITES[n_sites] else spd(rng, m, lo, 9.0 * lo)
        beliefs.append((J, rng.standard_normal(m), float(rng.standard_normal())))
    dims = np.array([m, 1, 1], np.int32)
    one = (np.ones((1, 1)), np.zeros(1), 0.0)
    packed = np.stack([np.concatenate([pack_record(*b), pack_record(*one), pack_record(*one)]) for b in beliefs])
    return beliefs, dims, np.array([0, 1], np.int32), np.array([0, 1, 2], np.int64), np.array([m - 1, 0], np.int32), packed
