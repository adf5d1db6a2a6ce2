"""The plane-split packed layout (csrc/pgbp_bs16.hpp: a tile's left block columns, then its right ones) through every kernel
that reads or writes it directly, at the smallest shapes at which a wrong permutation can hide: the clique trees of a 4-tip and
a 5-tip caterpillar tree (a cherry; a cluster with one leaf and one internal child; a constant below the root), random
symmetric positive-definite beliefs with all-distinct entries.

Tolerance: the one of tests/test_gpu_parity.py (1e-8 * max(1, |.|_inf) per belief, residuals to rtol 1e-8 / atol 1e-9) against
the numpy oracle; bitwise where two paths do the same arithmetic on the same layout.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import bs16_planes_cases as K
from helpers import oracle_cgb_from_problem, oracle_schedule
from oracle import calibration as OC

pytestmark = pytest.mark.gpu

RTOL = 1e-8


@pytest.fixture(scope="module")
def P():
    import pgbp_amd
    pgbp_amd.load()
    return pgbp_amd


def _assert_site_matches_oracle(eng, site, ocgb, prob, tag):
    eng.site = site
    for i, ob in enumerate(ocgb.belief):     # clusters and sepsets
        pb = eng.belief[i]
        for name, x, y in (("J", pb.J, ob.J), ("h", pb.h, ob.h), ("g", pb.g, ob.g)):
            x, y = np.asarray(x), np.asarray(y)
            if x.size == 0:
                continue
            scale = max(1.0, float(np.max(np.abs(y))))
            err = float(np.max(np.abs(x - y)))
            assert err <= RTOL * scale, f"{tag} site {site} belief {i} {name}: err {err:.3e} scale {scale:.3e}"
    for key, omr in ocgb.messageresidual.items():
        pmr = eng.messageresidual[key]
        assert np.allclose(pmr.dJ, omr.dJ, rtol=1e-8, atol=1e-9), (tag, site, key)
        assert np.allclose(pmr.dh, omr.dh, rtol=1e-8, atol=1e-9), (tag, site, key)
        assert pmr.iscalibrated_resid == omr.iscalibrated_resid, (tag, site, key)


def _calibrate_packed(P, prob, packs):
    """one calibrate! on the device; the packed path must be the one that ran"""
    eng = P.ClusterGraphBelief.from_arrays(prob.dims, prob.sepset_clusters, prob.scope_off, prob.scope_idx, np.stack(packs),
                                           n_sites=len(packs))
    assert P.calibrate_(eng, prob.schedule, 1, sync=False)[0]
    assert eng._lib.pgbp_layout(eng._eng) & 1, "the beliefs are expected in the packed layout after the calibration"
    eng.pull()
    return eng


@pytest.mark.parametrize("ntips", [4, 5])
@pytest.mark.parametrize("p", [2, 8, 16])
def test_cliquetree_against_the_oracle(P, ntips, p):
    """G = 1 (a plane is one block), G = 4 and G = 8: every belief, sepset and residual after one calibrate!"""
    prob, packs = K.cliquetree_case(ntips, p, 1)
    eng = _calibrate_packed(P, prob, packs)
    ocgb = oracle_cgb_from_problem(prob, packs[0], p)
    assert OC.calibrate(ocgb, [oracle_schedule(prob)], 1)[0]
    _assert_site_matches_oracle(eng, 0, ocgb, prob, f"cliquetree {ntips} tips p {p}")


@pytest.mark.parametrize("ntips", [4, 5])
def test_cliquetree_two_sites(P, ntips):
    """p = 16, two sites with different data (grid.y = site; the last site's records end the pool)"""
    p = 16
    prob, packs = K.cliquetree_case(ntips, p, 2)
    assert not np.array_equal(packs[0], packs[1])
    eng = _calibrate_packed(P, prob, packs)
    for s in range(2):
        ocgb = oracle_cgb_from_problem(prob, packs[s], p)
        assert OC.calibrate(ocgb, [oracle_schedule(prob)], 1)[0]
        _assert_site_matches_oracle(eng, s, ocgb, prob, f"cliquetree {ntips} tips p {p}")


def test_bethe_prologue_instances(P):
    """The Bethe graph of the 5-tip tree at p = 8: the records with a prologue (the message variable cluster -> factor fused
    into the factor's own send), which read X's tile and the sepset (X, F) in the packed layout.  Against the plain-C engine
    (the numpy oracle's helpers build clique trees only)."""
    from oracle import cengine
    prob, packs = K.bethe_case(5, 8)
    eng = _calibrate_packed(P, prob, packs)
    pa, ch = prob.schedule[0]
    ref = cengine.Engine(prob.dims, prob.sepset_clusters, prob.scope_off, prob.scope_idx, packs[0])
    assert ref.calibrate(pa, ch, 1, return_iscal=True)[0]
    want = ref.packed()
    for i in range(len(prob.dims)):
        x, y = eng._packed_raw[0, prob.packed_off[i]:prob.packed_off[i + 1]], want[prob.packed_off[i]:prob.packed_off[i + 1]]
        err, scale = float(np.max(np.abs(x - y))), max(1.0, float(np.max(np.abs(y))))
        assert err <= RTOL * scale, f"bethe belief {i}: err {err:.3e} scale {scale:.3e}"
    res, flags = ref.residuals()
    assert np.allclose(eng._res[0, :len(res)], res, rtol=1e-8, atol=1e-9)
    assert np.array_equal(eng._flg[0].astype(bool), flags.astype(bool))


def test_level_tail_and_loop_kernels_share_the_layout(P, tmp_path):
    """The 5-tip tree at p = 16 with the loop launches on one wavefront per record (loop=0: bp_fast16's own loop mode), without
    fused levels (no_chunks) and with the default plan, each in a child process: the three downloads are equal bit for bit."""
    here = os.path.dirname(os.path.abspath(__file__))
    outs = []
    for k, tuning in enumerate(["loop=0", "no_chunks", ""]):
        env = dict(os.environ)
        env.pop("PGBP_TUNING", None)
        if tuning:
            env["PGBP_TUNING"] = tuning
        path = str(tmp_path / f"out{k}.npz")
        out = subprocess.run([sys.executable, os.path.join(here, "run_bs16_planes_tree.py"), path], env=env,
                             capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, (tuning, out.stdout[-1500:], out.stderr[-1500:])
        outs.append(np.load(path))
        assert int(outs[-1]["layout"]) & 1, tuning
    for o in outs[1:]:
        for name in ("packed", "res", "flags"):
            assert np.array_equal(outs[0][name], o[name]), name
    assert np.abs(outs[0]["res"]).max() > 0.0


@pytest.mark.parametrize("p", [2, 8, 16])
def test_untouched_leaf_comes_back_bit_for_bit(P, p):
    """Upload -> one postorder (plain -> packed) -> pgbp_get_belief (packed -> plain) of the clusters that only send: the
    convert kernels against J_off."""
    from pgbp_amd import _lib as L
    prob, packs = K.cliquetree_case(5, p, 1)
    cgb = P.ClusterGraphBelief.from_arrays(prob.dims, prob.sepset_clusters, prob.scope_off, prob.scope_idx, packs[0])
    cgb.set_schedule(prob.schedule)
    assert P.propagate_1traversal_postorder_(cgb, None, None, *prob.schedule[0], sync=False)
    pa, ch = prob.schedule[0]
    leaves = [int(c) for c in ch if int(c) not in set(int(x) for x in pa) and prob.dims[c] > 0]
    assert len(leaves) >= 3
    for n, i in enumerate(leaves):
        assert n > 0 or cgb._lib.pgbp_layout(cgb._eng) & 1, "the beliefs are expected in the packed layout after the postorder"
        rec = np.zeros(int(prob.packed_off[i + 1] - prob.packed_off[i]))
        assert cgb._lib.pgbp_get_belief(cgb._eng, 0, i, L.f64p(rec)) == L.PGBP_OK
        assert np.array_equal(rec, packs[0][prob.packed_off[i]:prob.packed_off[i + 1]]), i
