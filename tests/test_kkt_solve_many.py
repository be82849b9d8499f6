"""Several right-hand sides through the chain KKT solver in one pass (iem_kkt_solve_many, csrc/iem_kkt_many_device.h) and
sensitivity.parameter_steps — the parts that need no device: the C-ABI surface, the multi-column kernels in every precompiled
shape's source (cross-compiled for gfx950, no scratch), the refusals that come before any device work, the levels with a
matrix right-hand side as a restatement against the dense restatement column by column (algebra only), and parameter_steps behind a counting dense solve."""
import ast
import ctypes as C
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import scipy.linalg
from scipy.sparse.linalg import spsolve

import cases
import chain_reference as ref
from pyoracle import OracleModel
from test_kkt import host_kkt
from test_kkt_chain import _system
from test_parameter_step import HostParamModel, ScipyKKT, TOL, _attached, _cores

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MANY_KERNELS = ["kkt_forward_m", "kkt_backward_m", "kkt_move_m", "kkt_colsum_m"]
ROW_KERNELS = ["kkt_fz_m", "kkt_fs_m", "kkt_bw_m"]


def build_shapes():
    """The (nb, ne, nc) shapes __graft_entry__.build() precompiles: read from its source, not copied."""
    tree = ast.parse(open(os.path.join(ROOT, "__graft_entry__.py")).read())
    for node in ast.walk(tree):
        if isinstance(node, ast.For) and isinstance(node.target, ast.Tuple) and [getattr(e, "id", None) for e in node.target.elts] == ["nb", "ne", "nc"]:
            return [tuple(s) for s in ast.literal_eval(node.iter)]
    raise AssertionError("build() no longer lists the chain KKT shapes in a `for nb, ne, nc in (...)` loop")


def test_solve_many_is_declared_exported_and_bound(built):
    from infiniteexamodels.jl_amd import lib as iemlib
    header = open(os.path.join(ROOT, "include", "iem.h")).read()
    for sym in ("iem_kkt_solve_many", "iem_kkt_chain_solve_many"):
        assert re.search(r"^int %s\(" % sym, header, re.M), sym
        assert sym in iemlib.SYMBOLS
    assert re.search(r"int iem_kkt_solve_many\(iem_kkt \*k, int nrhs, const double \*d_rhs, int64_t ld_rhs, double \*d_sol, int64_t ld_sol\);", header)
    exported = subprocess.check_output(["nm", "-D", "--defined-only", iemlib.LIB_PATH], text=True)
    assert " T iem_kkt_solve_many" in exported and " T iem_kkt_chain_solve_many" in exported
    L = iemlib.lib()
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int
    assert L.iem_kkt_solve_many.argtypes == [vp, i32, vp, i64, vp, i64]
    assert len(L.iem_kkt_chain_solve_many.argtypes) == len(L.iem_kkt_chain_solve_lanes.argtypes) + 1
    # the info struct did not grow (it has no size field)
    assert C.sizeof(iemlib.KktInfo) == 4 * 8 + 6 * 4 + 2 * 8 + 4 * 4


def test_refusals_before_any_device_work(built):
    from infiniteexamodels.jl_amd import lib as iemlib
    L = iemlib.lib()
    buf = (C.c_double * 8)()
    assert L.iem_kkt_solve_many(None, 1, buf, 8, buf, 8) == -4                      # IEM_E_ARG: null k
    assert b"null" in L.iem_last_error()
    assert L.iem_kkt_chain_solve_many(None, 4, 4, 20, 0, 4, buf, buf, buf, buf, buf, None, buf, buf, None, None, 2, 0) == -4
    # nrhs < 1 is refused before the object is looked at: any non-null pointer will do for k
    for nrhs in (0, -3):
        assert L.iem_kkt_solve_many(C.cast(buf, C.c_void_p), nrhs, buf, 8, buf, 8) == -4
        assert b"nrhs" in L.iem_last_error()


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_every_precompiled_shape_carries_the_kernels_without_scratch(tmp_path, built):
    """kkt_source(nb, ne, nc) of every shape build() lists holds the multi-column kernels, cross-compiles for gfx950, and no
    multi-column kernel uses scratch (the compiler's own resource-usage remarks)."""
    from infiniteexamodels.jl_amd import lib as iemlib
    shapes = build_shapes()
    assert len(shapes) >= 13 and (40, 0, 12) in shapes and (20, 0, 8) in shapes and (20, 112, 4) in shapes
    assert "kkt_forward_m" not in iemlib.emit_source(cases.build_core("quadrotor_5").to_blob())[0]      # a model's own source stays as it was

    def one(shape):
        src, _ = iemlib.kkt_source(*shape)
        assert "iem_kkt_many_device.h" in src
        R = iemlib.kkt_many_width(*shape)
        assert R in (2, 4, 8)
        hip = tmp_path / ("k_%d_%d_%d.hip" % shape)
        hip.write_text(src)
        flags = src.split("\n", 1)[0][len("// iem-flags:"):].split()
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
        return shape, R, usage

    with ThreadPoolExecutor(4) as ex:
        for shape, R, usage in ex.map(one, shapes):
            nb, ne, nc = shape
            want = MANY_KERNELS + (ROW_KERNELS if ne == 0 and nb <= 64 else [])
            for kern in want:
                assert kern in usage, (shape, kern)
                print(shape, "R", R, kern, usage[kern])
                assert usage[kern]["scratch"] == 0, (shape, kern, usage[kern])


def _solve_levels_many(Dinv, X, Y, Z, G, Gp, r, rB):
    """The levels of chain_reference.solve with a MATRIX right-hand side, in the order the multi-column kernels work: r is
    (K, S, nb), rB (K, ne) — every level visits a block ONCE and applies it to the K columns one after the other, with the
    numpy products chain_reference.solve itself uses (its own border arrays are one column wide, so the loop nest is
    restated here: levels outside, columns inside)."""
    S, nb, _ = Dinv.shape
    ne = Z.shape[2]
    K = r.shape[0]
    r = r.copy()
    rBp = np.zeros((K, S, ne))
    levels = []
    s = 1
    while s < S:
        levels.append(s)
        for j in range(0, S, 2 * s):
            p, q = j - s, j + s
            for u in range(K):
                if j > 0:
                    r[u, j] -= Y[p].T @ r[u, p]
                if q < S:
                    r[u, j] -= X[q].T @ r[u, q]
        for i in range(s, S, 2 * s):
            for u in range(K):
                rBp[u, i] = Z[i].T @ r[u, i]
        s *= 2
    xB = np.zeros((K, ne))
    for u in range(K):
        rBp[u, 0] = Z[0].T @ r[u, 0]
        xB[u] = np.linalg.solve(G - Gp.sum(0), rB[u] - rBp[u].sum(0)) if ne else np.zeros(0)
        r[u, 0] = Dinv[0] @ r[u, 0] - Z[0] @ xB[u]
    for s in reversed(levels):
        for i in range(s, S, 2 * s):
            for u in range(K):
                v = Dinv[i] @ r[u, i] - X[i] @ r[u, i - s] - Z[i] @ xB[u]
                if i + s < S:
                    v -= Y[i] @ r[u, i + s]
                r[u, i] = v
    return r, xB


@pytest.mark.parametrize("name", ["quadrotor_5", "hovercraft", "farmer_5", "opf_7", "pandemic_20x3"])
def test_levels_with_a_matrix_right_hand_side(name, built):
    """The ALGEBRA of the multi-column levels, on restatements only (no product code runs here — the kernels and the host
    path are covered by the bitwise tests of tests/test_gpu_kkt_solve_many.py): block visited once per level and applied to
    every column gives exactly the column-by-column solves of chain_reference.solve, and scipy's answer at the tolerance of
    tests/test_kkt_chain.py's single-column check."""
    from infiniteexamodels.jl_amd.kkt_chain import ChainLayout
    core, om, K, rhs0 = _system(name)
    jr, jc = om.jac_structure()
    L = ChainLayout(core.slabs, om.nvar, om.ncon, jr, jc)
    n = om.nvar + om.ncon
    rows = np.repeat(np.arange(n), np.diff(K.indptr))
    D, B, E, G = ref.fill_blocks(L, rows, K.indices, K.data)
    Dinv, X, Y, Z, Gp, _ = ref.factor(D, B, E)
    on, pos, border = L.positions()
    nk = 5
    RHS = np.column_stack([rhs0] + [np.random.default_rng(40 + u).standard_normal(n) for u in range(1, nk)])

    def pack(Bm):
        r = np.zeros((Bm.shape[1], L.S * L.nb)); r[:, pos] = Bm[on].T
        rB = np.zeros((Bm.shape[1], L.ne)); rB[:, :L.n_border] = Bm[border].T
        return r.reshape(-1, L.S, L.nb), rB

    def unpack(xs, xB):
        out = np.empty((n, xs.shape[0])); out[on] = xs.reshape(xs.shape[0], -1)[:, pos].T; out[border] = xB[:, :L.n_border].T
        return out

    def solve_many(Bm):
        return unpack(*_solve_levels_many(Dinv, X, Y, Z, G, Gp, *pack(Bm)))

    def solve_one(b):
        r, rB = pack(b[:, None])
        xs, xB = ref.solve(Dinv, X, Y, Z, G, Gp, r[0], rB[0])
        return unpack(xs[None], xB[None])[:, 0]

    sol = solve_many(RHS)
    for u in range(nk):
        np.testing.assert_array_equal(sol[:, u], solve_one(RHS[:, u]))             # exactly: same operations, same order
    np.testing.assert_array_equal(solve_many(RHS[:, [2, 0]])[:, 1], sol[:, 0])      # ... wherever the column sits
    sol = sol + solve_many(RHS - K @ sol)                                           # one refinement step, as ChainKKT.solve
    Kc = K.tocsc()
    for u in range(nk):
        want = spsolve(Kc, RHS[:, u])
        assert np.abs(K @ sol[:, u] - RHS[:, u]).max() <= 1e-8 * max(1.0, np.abs(RHS[:, u]).max())
        np.testing.assert_allclose(sol[:, u], want, rtol=1e-6, atol=1e-8 * max(1.0, np.abs(want).max()))


@pytest.mark.parametrize("name", ["quadrotor_11", "pfun"])
def test_parameter_steps_is_one_solve_for_all_directions(name, built):
    import torch
    from infiniteexamodels.jl_amd.sensitivity import parameter_step, parameter_steps
    core = _cores()[name]()
    blob = core.to_blob()
    om = OracleModel(blob)
    rng = np.random.default_rng(31)
    x = om.x0 + 0.1 * rng.standard_normal(om.nvar)
    y = rng.standard_normal(om.ncon)
    Kd = host_kkt(om, x, y, np.zeros(om.nvar), 1e-2, 1e-2, w=0.7).toarray()
    model = HostParamModel(core, blob)
    xt, yt = torch.from_numpy(x), torch.from_numpy(y)
    for nk in (3, 1):
        dth = 0.1 * rng.standard_normal((om.npar, nk))
        kkt = ScipyKKT(Kd)
        dX, dY = parameter_steps(model, kkt, xt, yt, torch.from_numpy(dth), obj_weight=0.7)
        assert kkt.calls == 1                                                        # ONE solve, whatever K is
        assert tuple(dX.shape) == (om.nvar, nk) and tuple(dY.shape) == (om.ncon, nk)
        kkt2 = ScipyKKT(Kd)
        lX, lY = parameter_steps(model, kkt2, xt, yt, [torch.from_numpy(dth[:, u].copy()) for u in range(nk)], obj_weight=0.7)
        assert kkt2.calls == 1
        np.testing.assert_array_equal(lX.numpy(), dX.numpy())                        # a list and a 2-D tensor: identical
        np.testing.assert_array_equal(lY.numpy(), dY.numpy())
        for u in range(nk):
            dx, dy = parameter_step(model, ScipyKKT(Kd), xt, yt, torch.from_numpy(dth[:, u].copy()), obj_weight=0.7)
            want = np.concatenate([dx.numpy(), dy.numpy()])
            got = np.concatenate([dX[:, u].numpy(), dY[:, u].numpy()])
            err = np.abs(got - want).max() / max(1.0, np.abs(want).max())
            print(name, nk, u, "relative difference to parameter_step", err)
            assert np.abs(want).max() > 0 and err <= TOL
    with pytest.raises(ValueError):
        parameter_steps(model, ScipyKKT(Kd), xt, yt, torch.zeros(om.npar, dtype=torch.float64))      # 1-D: that is parameter_step
    with pytest.raises(ValueError):
        parameter_steps(model, ScipyKKT(Kd), xt, yt, [])


def test_parameter_directions_stacks_parameter_direction(built):
    m, (P1, P2) = cases.rosenbrock()
    be = _attached(m)
    th0 = np.array(be.core.theta, copy=True)
    D = be.parameter_directions([(P1, -2.0), (P2, 3.5), (P2, 0.25)])
    np.testing.assert_array_equal(be.core.theta, th0)                                # θ untouched
    assert D.shape == (th0.size, 3)
    for u, (pref, val) in enumerate([(P1, -2.0), (P2, 3.5), (P2, 0.25)]):
        np.testing.assert_array_equal(D[:, u], be.parameter_direction(pref, val))
    m, (pf1, pf2) = cases.pfun()
    be = _attached(m)
    th0 = np.array(be.core.theta, copy=True)
    new = lambda t, s: np.cos(t) * s - 0.3   # noqa: E731
    D = be.parameter_directions([(pf2, new)])
    np.testing.assert_array_equal(be.core.theta, th0)
    np.testing.assert_array_equal(D[:, 0], be.parameter_direction(pf2, new))
    with pytest.raises(ValueError):
        be.parameter_directions([])
    with pytest.raises(KeyError):
        be.parameter_directions([(object(), 1.0)])
