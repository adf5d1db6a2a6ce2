"""The simulation sweep, host side: the comparators of tests/simulate_ref.py pinned before the device is compared with them,
the node topology factors.lg_families derives, the Philox restatement against the published known-answer vectors, the
moments of the normals the GPU test draws, and the host pieces of pgbp_lg_set_topology under the host sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import loo_ref as LR
import simulate_ref as SR
from shift_ref import family_nodes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "phylogaussianbeliefprop.jl_amd", "csrc")
TOL = 1e-8


@pytest.mark.parametrize("variant", SR.VARIANTS)
@pytest.mark.parametrize("which,p", SR.DENSE_CASES)
def test_reference_sweep_has_the_dense_moments(which, p, variant):
    """simulate_ref.simulate is linear in z, x = m + A z: m and A A' against densemvn.node_moments of the (wrapped) model on
    every case the device is compared on."""
    net, model, tbl, taxa = SR.oracle_case(which, p)
    ocgb, fam, data, kw = SR.oracle_table(net, model, tbl, taxa)
    w, shifts, noise, _ = SR.variant(net, ocgb, fam, kw, model, p, variant)
    m, A = SR.mean_and_map(fam, SR.site_kw(kw, 0, p, False), p, shifts, noise)
    em, ec = SR.moment_errors(m, A, net, w, family_nodes(ocgb, fam))
    print(f"{which}/p{p}/{variant}: {len(fam['cluster'])} families, mean {em:.2e}, A A' {ec:.2e}")
    assert em <= TOL and ec <= TOL
    if variant != "plain":   # the variant is not a no-op
        m0, A0 = SR.mean_and_map(fam, SR.site_kw(kw, 0, p, False), p)
        assert SR.rel(m0, m) > 1e-3 or SR.rel(A0 @ A0.T, A @ A.T) > 1e-3


@pytest.mark.parametrize("which,p", SR.DENSE_CASES + [("bm_improper", 2)])
def test_parent_family_is_the_family_of_the_parent_node(which, p):
    """lg_families' parent_family against shift_ref.family_nodes and the oracle's node2family: -1 under a fixed root, -2 under
    an improper one, parents before their children."""
    net, model, tbl, taxa = SR.oracle_case(which, p)
    ocgb, fam, _, _ = SR.oracle_table(net, model, tbl, taxa)
    nodes = family_nodes(ocgb, fam)
    K = max(1, int(fam["max_parents"]))
    pf = np.asarray(fam["parent_family"]).reshape(len(nodes), K)
    improper = bool(np.any(np.isinf(np.diag(np.atleast_2d(np.asarray(model.rootpriorvariance(), float))))))
    seen = set()
    for f, i in enumerate(nodes):
        for k in range(int(fam["n_parents"][f])):
            pi = ocgb.node2family[i][1 + k] - 1
            want = nodes.index(pi) if pi in nodes else (-1 if model.isrootfixed() else -2)
            assert pf[f, k] == want and want < f, (f, k, pf[f, k], want)
            seen.add(want)
    assert (-1 in seen) == bool(model.isrootfixed()) and (-2 in seen) == improper
    if improper:
        with pytest.raises(ValueError, match="improper"):
            SR.simulate(fam, dict(R=np.zeros((2, p, p)), mu=np.zeros(p)), np.zeros((len(nodes), p)), p)


def test_philox_known_answers():
    """Philox4x32-10 against the known-answer vectors published with the generator (Random123, kat_vectors)."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    ctr = np.array([c for c, _, _ in kat], np.uint64)
    key = np.array([k for _, k, _ in kat], np.uint64)
    got = SR.philox4x32_10(ctr, key)
    assert got.tolist() == [list(o) for _, _, o in kat], [[hex(int(v)) for v in r] for r in got]


def test_uniforms_and_normals_of_the_gpu_seed():
    """The 2^17 normals the GPU moment test draws: mean and variance within 5 standard errors (so that test cannot fail for
    statistical reasons); the uniforms lie in (0, 1]; a draw depends on (site, family, trait) only; odd p drops the last sine."""
    s, nf, p = SR.MOMENT_SHAPE
    z = SR.normals(SR.SEED, np.arange(s), nf, p).reshape(-1)[: 1 << 17]
    assert z.size == 1 << 17 and np.all(np.isfinite(z)) and float(np.max(np.abs(z))) < 9.0
    em, ev = SR.moment_band(z)
    print(f"2^17 normals of seed {SR.SEED:#x}: |mean| {em:.2f} s.e., |var - 1| {ev:.2f} s.e.")
    assert em <= 5.0 and ev <= 5.0
    u = SR.uniform53(np.array([0, 0xFFFFFFFF], np.uint64), np.array([0, 0xFFFFFFFF], np.uint64))
    assert u[0] == 2.0 ** -54 and u[1] == 1.0
    a = SR.normals(SR.SEED, [5, 9], 4, 3)
    b = SR.normals(SR.SEED, [9], 7, 4)
    assert np.array_equal(a[1, :, :2], b[0, :4, :2]) and not np.array_equal(a[0], a[1])
    assert np.array_equal(SR.normals(SR.SEED, [9], 4, 2)[0], b[0, :4, :2])


def test_topology_host_pieces_under_the_sanitizers(tmp_path):
    """tests/topology_check.cpp over csrc/pgbp_topology.cpp, built with -fsanitize=address,undefined, as a process of its own."""
    if shutil.which("g++") is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "topology_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "topology_check.cpp"),
                           os.path.join(CSRC, "pgbp_topology.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert out.returncode == 0, out.stdout
    lines = out.stdout.splitlines()
    for what in ("random root levels", "fixed root levels", "improper root", "parent after its child", "outputs untouched",
                 "empty table"):
        assert "ok " + what in lines, out.stdout
    assert lines[-1] == "topology ok", out.stdout
