"""The dense border of the chain KKT solver on the device (csrc/iem_kkt_border_device.h) — the parts that need no device: the
numpy restatement of the two kernels (tests/border_reference.py) against numpy's eigenvalues and LU solve on every matrix family,
the C-ABI surface, the refusals that come before any device work, and the source cross-compiled for gfx950 without scratch."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import border_reference as br
import cases
import chain_reference as ref
from pyoracle import OracleModel
from test_kkt_chain import _system

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["iem_kkt_border_factor", "iem_kkt_border_solve", "iem_kkt_border_source", "iem_kkt_set_border", "iem_kkt_factor_async"]
ratios = []      # the backward-error ratios seen (printed by the last test; the largest is recorded in DESIGN.md)


def backward_error(G, x, r):
    return np.abs(r - G @ x).max() / (np.abs(G).sum(axis=1).max() * np.abs(x).max() + np.abs(r).max())


def check_solution(G, F, piv, seed, what):
    """normwise backward error of the restated solve at most 16 × numpy.linalg.solve's on the same system (floor 2⁻⁵³)"""
    r = np.random.default_rng(seed).standard_normal(G.shape[0])
    mine, lu = backward_error(G, br.solve(F, piv, r), r), backward_error(G, np.linalg.solve(G, r), r)
    ratio = mine / max(lu, 2.0 ** -53)
    ratios.append(ratio)
    print(what, "backward error", mine, "numpy", lu, "ratio", ratio)
    assert ratio <= 16.0, (what, mine, lu)


def check_factors(G, F, piv):
    """P Gs Pᵀ = L D Lᵀ with the documented storage"""
    n = G.shape[0]
    perm, typ = br.decode(piv)
    assert sorted(perm) == list(range(n))
    L, D = np.tril(F, -1) + np.eye(n), np.diag(np.diag(F)).copy()
    for i in range(n):
        if typ[i] == 1:
            assert typ[i + 1] == 2
            D[i + 1, i] = D[i, i + 1] = F[i + 1, i]
            L[i + 1, i] = 0.0
    assert np.abs(L @ D @ L.T - G[np.ix_(perm, perm)]).max() <= 1e-12 * n * np.abs(G).max()


@pytest.mark.parametrize("n", [3, 10, 61, 66, 125])
def test_quasi_definite(n):
    """(a) [A Bᵀ; B −C], A and C SPD: the inertia is known — and numpy's"""
    for seed in range(3):
        M, q = br.quasi_definite(n, seed)
        G = br.pad(M, n + 3)
        F, piv, neg, dbt, n2 = br.ldl(G)
        assert (neg, dbt) == (q, 0) and neg == int((np.linalg.eigvalsh(G) < 0).sum())
        check_factors(G, F, piv)
        check_solution(G, F, piv, seed, ("a", n, seed))


@pytest.mark.parametrize("n", [4, 10, 60, 66, 124])
def test_saddle_points_take_2x2_pivots(n):
    """(b) [0 B; Bᵀ 0] + a small perturbation: 2 × 2 pivots, (k, k, 0); the host path's LDLᵀ rule calls the unperturbed matrix doubtful"""
    for seed in range(3):
        M0, M, h = br.saddle(n, seed)
        F, piv, neg, dbt, n2 = br.ldl(M)
        assert n2 >= 1 and (n - neg - dbt, neg, dbt) == (h, h, 0)
        assert neg == int((np.linalg.eigvalsh(M) < 0).sum())
        check_factors(M, F, piv)
        check_solution(M, F, piv, seed, ("b", n, seed))
        assert br.sym_inertia_ldl(M0)[1] > 0                      # no 2 × 2 pivots there: a zero diagonal is doubtful
        assert br.ldl(M0)[2:4] == (h, 0) and br.ldl(M0)[4] == h   # ... while every pivot of the restatement is 2 × 2 on it


def test_exactly_singular_is_doubtful_never_positive():
    """(c) [[2,1,3],[1,1,2],[3,2,5]] (row 3 = row 1 + row 2; the elimination is exact) in a padded 4 × 4, and copies of it"""
    F, piv, neg, dbt, n2 = br.ldl(br.pad(br.SINGULAR3, 4))
    assert (neg, dbt, n2) == (0, 1, 0)
    assert 4 - neg - dbt == int((np.linalg.eigvalsh(br.pad(br.SINGULAR3, 4)) > 1e-12).sum())      # the zero eigenvalue is not among the positive
    assert abs(F[2, 2]) == 1e-14 * 5.0 and np.isfinite(F).all()
    for n, ne in ((10, 12), (61, 64), (125, 128)):
        G = br.pad(br.singular(n), ne)
        F, piv, neg, dbt, n2 = br.ldl(G)
        assert (neg, dbt) == (0, n // 3)
        assert ne - neg - dbt == int((np.linalg.eigvalsh(G) > 1e-12).sum())
    assert br.ldl(np.zeros((4, 4)))[2:4] == (0, 4)      # scale == 0: every step doubtful


@pytest.mark.parametrize("name", ["farmer_5", "opf_7", "pandemic_20x3", "pandemic_100x7"])
def test_schur_complements_of_the_models(name, built):
    """(d) Gs = G − Σ Gp of the models' blocks (tests/chain_reference.py).  The layout keeps pandemic_20x3 as ONE chain of 52 × 52
    blocks without a border (ne = 0: its Schur complement is the empty matrix, which must pass through as such); pandemic_100x7 is
    the pandemic grid that does have one (lanes, u(t) in a border of 100)."""
    Gs = model_border(name)
    assert Gs.shape[0] == {"farmer_5": 4, "opf_7": 52, "pandemic_20x3": 0, "pandemic_100x7": 100}[name]
    F, piv, neg, dbt, n2 = br.ldl(Gs)
    if not Gs.size:
        assert (neg, dbt, n2, len(piv)) == (0, 0, 0, 0) and br.solve(F, piv, np.zeros(0)).size == 0
        return
    assert (neg, dbt) == (int((np.linalg.eigvalsh(Gs) < 0).sum()), 0)
    check_factors(Gs, F, piv)
    check_solution(Gs, F, piv, 4, ("d", name))


def model_border(name):
    from infiniteexamodels.jl_amd.kkt_chain import ChainLayout
    core, om, K, rhs = _system(name)
    jr, jc = om.jac_structure()
    L = ChainLayout(core.slabs, om.nvar, om.ncon, jr, jc)
    rows = np.repeat(np.arange(om.nvar + om.ncon), np.diff(K.indptr))
    D, B, E, G = ref.fill_blocks(L, rows, K.indices, K.data)
    Gp = ref.factor(D, B, E)[4]
    assert G.shape == (L.ne, L.ne)
    Gs = G - br.colsum(Gp.reshape(L.S, -1)).reshape(G.shape)
    # Σ Gp is symmetric only up to the rounding of E'Z; the factorisation reads the LOWER triangle (that is the matrix it
    # factorises and solves with), so the checks are made against the lower triangle mirrored
    # (the two triangles differ by up to 1e-11 of the largest entry here: the pivot blocks carry 1 / delta_c = 1e6)
    return np.tril(Gs) + np.tril(Gs, -1).T


def test_the_column_sum_is_kkt_colsum():
    rng = np.random.default_rng(2)
    for rows in (1, 3, 512, 513, 700, 1025):
        a = rng.standard_normal((rows, 5))
        per = (rows + 511) // 512
        want = np.zeros(5)
        for c in range(0, rows, per):
            acc = np.zeros(5)
            for r in range(c, min(c + per, rows)):
                acc += a[r]
            want += acc
        assert np.array_equal(br.colsum(a), want)
        np.testing.assert_allclose(br.colsum(a), a.sum(axis=0), atol=1e-12)


def test_declared_exported_and_bound(built):
    from infiniteexamodels.jl_amd import lib as iemlib
    header = open(os.path.join(ROOT, "include", "iem.h")).read()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", iemlib.LIB_PATH], text=True)
    L = iemlib.lib()
    for sym in NEW:
        assert re.search(r"^int %s\(" % sym, header, re.M), sym
        assert sym in iemlib.SYMBOLS and " T %s\n" % sym in exported
        assert getattr(L, sym).argtypes is not None
    vp, i64, i32, dbl = C.c_void_p, C.c_int64, C.c_int, C.c_double
    assert L.iem_kkt_border_factor.argtypes == [vp, i64, i32, i32, vp, vp, vp, vp, vp, dbl]
    assert L.iem_kkt_border_solve.argtypes == [vp, i64, i32, i32, i32, vp, vp, vp, vp, vp]
    assert L.iem_kkt_set_border.argtypes == [vp, i32] and L.iem_kkt_factor_async.argtypes == [vp, vp]
    julia = open(os.path.join(ROOT, "infiniteexamodels.jl_amd", "julia", "MI355XBackend.jl")).read()
    for sym in ("iem_kkt_border_factor", "iem_kkt_border_solve", "iem_kkt_set_border", "iem_kkt_factor_async"):
        assert ":%s," % sym in julia, sym
    src, key = iemlib.kkt_border_source()
    assert src.startswith("// iem-flags: -O3 -ffp-contract=off") and "kkt_border_ldl" in src and "kkt_border_solve" in src
    assert os.path.exists(os.path.join(iemlib.KERNEL_DIR, "iem_%016x.hsaco" % key)), "build() precompiles the border's code object"


def test_refusals_before_any_device_work(built):
    """a null handle with otherwise valid arguments and a bad shape with a handle that is not one: both IEM_E_ARG, nothing touched"""
    from infiniteexamodels.jl_amd import lib as iemlib
    L = iemlib.lib()
    buf = (C.c_double * 16)()
    fake = C.cast(buf, C.c_void_p)      # never dereferenced: the shape is judged first
    assert L.iem_kkt_border_factor(None, 1, 4, 3, buf, buf, buf, buf, buf, 1e-14) == -4
    assert L.iem_kkt_border_solve(None, 1, 4, 3, 1, buf, buf, buf, buf, buf) == -4
    for S, ne, nb_ in ((1, 0, 0), (1, 6, 2), (1, 2, 2), (1, 132, 4), (1, 8, 9), (1, 8, -1), (0, 8, 4)):
        assert L.iem_kkt_border_factor(fake, S, ne, nb_, buf, buf, buf, buf, buf, 1e-14) == -4, (S, ne, nb_)
        assert b"multiple of 4" in L.iem_last_error()
        assert L.iem_kkt_border_solve(fake, S, ne, nb_, 1, buf, buf, buf, buf, buf) == -4, (S, ne, nb_)
    assert L.iem_kkt_border_solve(fake, 1, 8, 4, 0, buf, buf, buf, buf, buf) == -4 and b"nrhs" in L.iem_last_error()
    assert L.iem_kkt_border_factor(fake, 1, 8, 4, buf, None, buf, buf, buf, 1e-14) == -4
    assert L.iem_kkt_set_border(None, 1) == -4 and L.iem_kkt_set_border(fake, 2) == -4 and L.iem_kkt_set_border(fake, -1) == -4
    assert L.iem_kkt_factor_async(None, buf) == -4 and L.iem_kkt_factor_async(fake, None) == -4


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_the_source_cross_compiles_without_scratch(tmp_path, built):
    from infiniteexamodels.jl_amd import lib as iemlib
    src, _ = iemlib.kkt_border_source()
    hip = tmp_path / "border.hip"
    hip.write_text(src)
    flags = src.split("\n", 1)[0][len("// iem-flags:"):].split()
    assert "-ffp-contract=off" in flags
    p = subprocess.run(["/opt/rocm/bin/hipcc", "--genco", "--offload-arch=gfx950", *flags, "-Rpass-analysis=kernel-resource-usage",
                        "-o", str(hip) + ".hsaco", str(hip)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    usage, cur = {}, None
    for m in re.finditer(r"Function Name: (\S+)|ScratchSize \[bytes/lane\]: (\d+)|VGPRs: (\d+)", p.stderr):
        if m.group(1):
            cur = m.group(1)
        elif m.group(2) is not None:
            usage.setdefault(cur, {})["scratch"] = int(m.group(2))
        elif m.group(3) is not None:
            usage.setdefault(cur, {}).setdefault("vgprs", int(m.group(3)))
    print(usage)
    for kern in ("kkt_border_ldl", "kkt_border_solve", "kkt_border_colsum", "kkt_border_inertia"):
        assert usage[kern]["scratch"] == 0, (kern, usage[kern])
    # the LDS the host asks for at the largest border fits a CU (the formula of include/iem.h and DESIGN.md)
    assert 8 * (128 * 129 + 2 * 128 + 16) + 4 * (2 * 128 + 16) == 135360 <= 160 * 1024


def test_largest_ratio_seen():
    print("largest backward-error ratio against numpy.linalg.solve:", max(ratios) if ratios else None)
    assert not ratios or max(ratios) <= 16.0
