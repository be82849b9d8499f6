"""The dense border on the MI355X: iem_kkt_border_factor / _solve bitwise against the numpy restatement (tests/border_reference.py),
the solver object in mode 1 (iem_kkt_set_border) against mode 0 and scipy, and what mode 1 makes possible — assemble + factor +
refined solve of a bordered model captured as ONE graph."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import border_reference as br
import cases
from pyoracle import OracleModel
from test_kkt import host_kkt

pytestmark = pytest.mark.gpu
DW, DC = 1e-2, 1e-6
# delta_c of the comparison with mode 0.  Mode 0 calls an eigenvalue of the border's Schur complement doubtful below 1e-14 of the
# largest one; on opf_600 that one is 1.5e8 at delta_c = 1e-6 (600 scenarios' terms over delta_c), so mode 0 cannot certify the
# border's own -delta_c rows there (numpy on the blocks of tests/chain_reference.py: ten eigenvalues of -1e-6 under a threshold of
# 1.5e-6).  At 1e-4 the largest eigenvalue is 1.5e6 and the threshold 1.5e-8: both modes can count every pivot of every model.
DC_CMP = 1e-4
E_ARG = -4


def _bits(t):
    import torch
    return t.view(torch.int64)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def nan(*shape):
    import torch
    return torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")


# ---- the low-level pair against the restatement ---------------------------------------------------------------------------------
SHAPES = [(4, 3, 1), (12, 10, 3), (64, 61, 700), (68, 66, 3), (128, 125, 1)]      # (ne, n_border, S); 700 blocks: beyond the column sum's 512 row chunks


def family(which, ne, nb_):
    if which == "a":
        return br.pad(br.quasi_definite(nb_, 11)[0], ne)
    if which == "b":
        return br.pad(br.saddle(nb_ - nb_ % 2, 12)[1], ne)
    return br.pad(br.singular(nb_), ne)


_low = {}


def low_case(which, ne, nb_, S):
    """(G, Gp, rB, rBp, expected F, piv, neg, doubtful, 2x2 pivots, xB for 5 columns): computed once, shared and left unchanged"""
    key = (which, ne, nb_, S)
    if key not in _low:
        rng = np.random.default_rng(1000 * ne + S)
        M = family(which, ne, nb_)
        if which == "c":      # integer terms: G − Σ Gp is the singular matrix exactly
            Gp = rng.integers(-2, 3, size=(S, ne, ne)).astype(np.float64)
        else:
            Gp = rng.standard_normal((S, ne, ne)) / S
        Gp = Gp + Gp.transpose(0, 2, 1)
        gsum = br.colsum(Gp.reshape(S, ne * ne))
        G = M + gsum.reshape(ne, ne)
        F, piv, neg, dbt, n2 = br.ldl(G, gsum)
        rB = rng.standard_normal((5, ne))
        rB[:, nb_:] = np.nan      # never read: the padding's right-hand side is zero
        rBp = rng.standard_normal((5, S, ne))
        xB = np.stack([br.solve(F, piv, br.border_rhs(rB[u], rBp[u], ne, nb_)) for u in range(5)])
        _low[key] = (G, Gp, rB, rBp, F, piv, neg, dbt, n2, xB)
    return _low[key]


@pytest.fixture(scope="module")
def handle(built):
    from infiniteexamodels.jl_amd.model import ExaModel
    core = cases.build_core("farmer_5")
    gm = ExaModel(core, device=0, blob=core.to_blob())
    yield gm
    gm.close()


@pytest.mark.parametrize("which", ["a", "b", "c"])
@pytest.mark.parametrize("ne,nb_,S", SHAPES)
def test_low_level_calls_are_the_restatement_bit_for_bit(ne, nb_, S, which, handle):
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib
    gm = handle
    L = gm._L
    G, Gp, rB, rBp, F, piv, neg, dbt, n2, xB = low_case(which, ne, nb_, S)
    if which == "b":
        assert n2 >= 1 and dbt == 0
    if which == "c":
        assert dbt >= 1
    Gd, Gpd = torch.tensor(G, device="cuda"), torch.tensor(Gp, device="cuda")
    first = None
    for rep in range(10):
        Fd = nan(ne, ne)
        pd = torch.full((ne,), -2 ** 31, dtype=torch.int32, device="cuda")
        info = torch.tensor([5, 7, 0], dtype=torch.int64, device="cuda")
        gm._sync_stream()
        iemlib.check(L.iem_kkt_border_factor(gm._h, S, ne, nb_, _p(Gd), _p(Gpd), _p(Fd), _p(pd), _p(info), 1e-14))
        outs = [Fd, pd, info]
        for nrhs in (1, 5):
            xd = nan(nrhs, ne)
            rBpd, rBd = torch.tensor(rBp[:nrhs], device="cuda"), torch.tensor(rB[:nrhs], device="cuda")
            iemlib.check(L.iem_kkt_border_solve(gm._h, S, ne, nb_, nrhs, _p(Fd), _p(pd), _p(rBpd), _p(rBd), _p(xd)))
            outs += [xd, rBpd, rBd]
        torch.cuda.synchronize()
        outs = [o.cpu().numpy() for o in (outs[0], outs[1], outs[2], outs[3], outs[6])]
        if first is None:
            first = outs
            assert np.array_equal(outs[0].view(np.int64), F.view(np.int64)), np.argwhere(outs[0] != F)[:5]
            assert np.array_equal(outs[1], piv), (outs[1], piv)
            assert outs[2].tolist() == [5 + neg, 7 + dbt, 0]
            assert np.array_equal(outs[3].view(np.int64), xB[:1].view(np.int64)), np.abs(outs[3] - xB[:1]).max()
            assert np.array_equal(outs[4].view(np.int64), xB.view(np.int64)), np.abs(outs[4] - xB).max()
        else:
            for a, b in zip(outs, first):
                assert np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a, b.view(np.int64) if b.dtype == np.float64 else b), rep


def test_low_level_refusals(handle):
    import torch
    gm = handle
    L = gm._L
    z = torch.zeros(128 * 128, dtype=torch.float64, device="cuda")
    pv = torch.zeros(128, dtype=torch.int32, device="cuda")
    info = torch.zeros(3, dtype=torch.int64, device="cuda")
    for S, ne, nb_ in ((1, 0, 0), (1, 6, 2), (1, 132, 4), (1, 8, 9), (1, 8, -1), (0, 8, 4)):
        assert L.iem_kkt_border_factor(gm._h, S, ne, nb_, _p(z), _p(z), _p(z), _p(pv), _p(info), 1e-14) == E_ARG, (S, ne, nb_)
        assert L.iem_kkt_border_solve(gm._h, S, ne, nb_, 1, _p(z), _p(pv), _p(z), _p(z), _p(z)) == E_ARG, (S, ne, nb_)
    assert L.iem_kkt_border_solve(gm._h, 1, 8, 4, 0, _p(z), _p(pv), _p(z), _p(z), _p(z)) == E_ARG
    assert L.iem_kkt_border_factor(gm._h, 1, 8, 4, None, _p(z), _p(z), _p(pv), _p(info), 1e-14) == E_ARG


# ---- the object in mode 1 ---------------------------------------------------------------------------------------------------------
_host = {}


def host(name, dc=DC):
    """(core, blob, oracle, per seed: x, y, sigma, K of scipy, rhs): built once per model and delta_c, shared by the tests and left unchanged"""
    if dc != DC:
        if (name, dc) not in _host:
            core, blob, om, pts = host(name)
            _host[(name, dc)] = (core, blob, om, [(x, y, sigma, host_kkt(om, x, y, sigma, DW, dc), rhs) for x, y, sigma, _, rhs in pts])
        return _host[(name, dc)]
    if name not in _host:
        core = cases.build_core(name)
        blob = core.to_blob()
        om = OracleModel(blob)
        rng = np.random.default_rng(3)
        pts = []
        for seed in (5, 9):
            x, y = cases.eval_point_for(name, om, seed)
            sigma = 0.5 + rng.random(om.nvar)
            pts.append((x, y, sigma, host_kkt(om, x, y, sigma, DW, DC), rng.standard_normal(om.nvar + om.ncon)))
        _host[name] = (core, blob, om, pts)
    return _host[name]


@contextlib.contextmanager
def solver(name):
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.model import ExaModel
    core = _host[name][0] if name in _host else cases.build_core(name)
    gm = ExaModel(core, device=0, blob=_host[name][1] if name in _host else core.to_blob())
    k = C.c_void_p()
    iemlib.check(gm._L.iem_kkt_create(gm._h, 0, C.byref(k)))
    try:
        yield gm, k
    finally:
        iemlib.check(gm._L.iem_kkt_destroy(k))
        gm.close()


def values(gm, pt):
    import torch
    x, y, sigma = pt[:3]
    xd, yd, sd = (torch.tensor(a, device="cuda") for a in (x, y, sigma))
    hv, jv = gm.hess_coord(xd, yd, obj_weight=1.0).clone(), gm.jac_coord(xd).clone()
    gm._sync_stream()
    return xd, yd, sd, hv, jv


def factor(gm, k, hv, jv, sd, dw=DW, dc=DC):
    from infiniteexamodels.jl_amd import lib as iemlib
    iemlib.check(gm._L.iem_kkt_assemble(k, _p(hv), _p(jv), _p(sd), dw, dc))
    inertia = (C.c_int64 * 3)()
    iemlib.check(gm._L.iem_kkt_factor(k, inertia))
    return tuple(inertia)


def solve(gm, k, rhs, sol):
    from infiniteexamodels.jl_amd import lib as iemlib
    iemlib.check(gm._L.iem_kkt_solve(k, _p(rhs), _p(sol)))
    return sol


@pytest.mark.parametrize("name", ["farmer_5", "opf_7", "pandemic_20x3", "pandemic_100x7", "opf_600"])
def test_object_in_mode_1(name, built):
    """inertia equal to mode 0's; solutions against scipy with the tolerances of test_assemble_factor_solve_through_the_c_abi;
    iem_kkt_solve_many column for column bitwise iem_kkt_solve; back in mode 0 the bits of mode 0 before the switch."""
    import torch
    from scipy.sparse.linalg import spsolve
    from infiniteexamodels.jl_amd import lib as iemlib
    core, blob, om, pts = host(name, DC_CMP)
    n = om.nvar + om.ncon
    with solver(name) as (gm, k):
        L = gm._L
        info = iemlib.KktInfo()
        iemlib.check(L.iem_kkt_info(k, C.byref(info)))
        assert not info.hubs and (info.ne > 0) == (name != "pandemic_20x3")      # (that grid is one chain of 52 x 52 blocks without a border: the switch is a no-op)
        for pt in pts:
            x, y, sigma, Kh, rhs = pt
            xd, yd, sd, hv, jv = values(gm, pt)
            rd = torch.tensor(rhs, device="cuda")
            in0 = factor(gm, k, hv, jv, sd, DW, DC_CMP)
            sol0 = solve(gm, k, rd, nan(n)).clone()
            iemlib.check(L.iem_kkt_set_border(k, 1))
            if info.ne > 0:      # the switch invalidates
                assert L.iem_kkt_solve(k, _p(rd), _p(nan(n))) == E_ARG and "factorisation" in L.iem_last_error().decode()
            in1 = factor(gm, k, hv, jv, sd, DW, DC_CMP)
            print(name, "inertia mode 0", in0, "mode 1", in1)
            assert in1 == in0 and in1[2] == 0, (in0, in1)
            sol = solve(gm, k, rd, nan(n))
            xs = sol.cpu().numpy()
            res = rhs - Kh @ xs                      # one step of refinement, the residual formed on the host here
            rd2 = torch.tensor(res, device="cuda")
            solve(gm, k, rd2, rd2)                   # in place: the right-hand side is read before the solution is written
            xs = xs + rd2.cpu().numpy()
            want = spsolve(Kh.tocsc(), rhs)
            resid = np.abs(Kh @ xs - rhs)
            print(name, "residual", resid.max())
            assert resid.max() <= 1e-9 * max(1.0, np.abs(rhs).max()) or (resid / (abs(Kh) @ np.abs(xs) + np.abs(rhs))).max() <= 1e-12, name
            np.testing.assert_allclose(xs, want, rtol=1e-6, atol=1e-8 * max(1.0, np.abs(want).max()))
            # five columns (a full chunk and a rest), with a leading dimension of their own
            R = torch.tensor(np.random.default_rng(17).standard_normal((5, n + 3)), device="cuda")
            R[0, :n] = rd
            X = nan(5, n + 1)
            iemlib.check(L.iem_kkt_solve_many(k, 5, _p(R), n + 3, _p(X), n + 1))
            for u in range(5):
                assert torch.equal(_bits(X[u, :n]), _bits(solve(gm, k, R[u, :n].contiguous(), nan(n)))), (name, u)
            assert torch.equal(_bits(X[0, :n]), _bits(sol)) and torch.isnan(X[:, n]).all()
            # back to the host path: what it gave before
            iemlib.check(L.iem_kkt_set_border(k, 0))
            assert factor(gm, k, hv, jv, sd, DW, DC_CMP) == in0
            assert torch.equal(_bits(solve(gm, k, rd, nan(n))), _bits(sol0))


def test_small_regularisation_on_many_scenarios(built):
    """opf_600 at delta_c = 1e-6, the point of test_assemble_factor_solve_through_the_c_abi: the border's Schur complement has ten
    eigenvalues of -1e-6 (its own -delta_c rows) beside a largest one of 1.5e8.  Mode 0 reports them as doubtful (measured:
    (14434, 20418, 10)); the device's LDL' takes them as pivots of 1.0e-6 .. 1.1e-5 above its threshold 1e-14 max|Gs_ij| = 9.9e-7
    and counts them negative: (nvar, ncon, 0) = (14424, 20428, 0) — the count of numpy's eigenvalues on the restated blocks
    (20 400 negative block pivots + 28 negative eigenvalues of the 52 x 52 Schur complement).  The solution passes the same bounds."""
    import torch
    from scipy.sparse.linalg import spsolve
    from infiniteexamodels.jl_amd import lib as iemlib
    core, blob, om, pts = host("opf_600")
    n = om.nvar + om.ncon
    with solver("opf_600") as (gm, k):
        x, y, sigma, Kh, rhs = pts[0]
        xd, yd, sd, hv, jv = values(gm, pts[0])
        in0 = factor(gm, k, hv, jv, sd)
        iemlib.check(gm._L.iem_kkt_set_border(k, 1))
        in1 = factor(gm, k, hv, jv, sd)
        print("opf_600 at delta_c = 1e-6: mode 0", in0, "mode 1", in1)
        assert in1 == (om.nvar, om.ncon, 0)
        assert in0[1] + in0[2] == in1[1]      # what mode 0 could not certify are those negative pivots
        rd = torch.tensor(rhs, device="cuda")
        xs = solve(gm, k, rd, nan(n)).cpu().numpy()
        rd2 = torch.tensor(rhs - Kh @ xs, device="cuda")
        solve(gm, k, rd2, rd2)
        xs = xs + rd2.cpu().numpy()
        want = spsolve(Kh.tocsc(), rhs)
        resid = np.abs(Kh @ xs - rhs)
        assert resid.max() <= 1e-9 * max(1.0, np.abs(rhs).max()) or (resid / (abs(Kh) @ np.abs(xs) + np.abs(rhs))).max() <= 1e-12
        np.testing.assert_allclose(xs, want, rtol=1e-6, atol=1e-8 * max(1.0, np.abs(want).max()))


def test_a_singular_border_is_doubtful_in_mode_1(built):
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib
    core, blob, om, pts = host("farmer_5")
    with solver("farmer_5") as (gm, k):
        iemlib.check(gm._L.iem_kkt_set_border(k, 1))
        xd, yd, sd, hv, jv = values(gm, pts[0])
        zero = torch.zeros_like(sd)
        inertia = factor(gm, k, hv, jv, zero, 0.0, 0.0)
        assert inertia[2] > 0, inertia
        inertia = factor(gm, k, hv, jv, zero, DW, DC)      # regularised, the same object factorises cleanly again
        assert (inertia[1], inertia[2]) == (om.ncon, 0), inertia


@pytest.mark.parametrize("name", ["opf_7", "pandemic_20x3"])
def test_newton_step_of_a_bordered_model_is_one_graph(name, built):
    """assemble + iem_kkt_factor_async + iem_kkt_solve_refined(steps = 1) captured after a warm-up call; two replays with new
    hess / jac values in the same buffers, each bitwise the eager calls (solution, norms, device inertia)."""
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib
    core, blob, om, pts = host(name)
    n = om.nvar + om.ncon
    with solver(name) as (gm, k):
        L = gm._L
        iemlib.check(L.iem_kkt_set_border(k, 1))
        rd = torch.tensor(pts[0][4], device="cuda")
        vals = [values(gm, pt) for pt in pts]
        xd, yd, sd, hv, jv = (t.clone() for t in vals[0])

        def step(sol, norms, inert):
            iemlib.check(L.iem_kkt_assemble(k, _p(hv), _p(jv), _p(sd), DW, DC))
            iemlib.check(L.iem_kkt_factor_async(k, _p(inert)))
            iemlib.check(L.iem_kkt_solve_refined(k, _p(xd), _p(yd), 1.0, _p(sd), DW, DC, _p(rd), _p(sol), 1, _p(norms)))

        def load(i):
            for dst, src in zip((xd, yd, sd, hv, jv), vals[i]):
                dst.copy_(src)

        eager = []
        for i in (0, 1, 0):      # (the first of them is the warm-up as well)
            load(i)
            sol, norms, inert = nan(n), nan(2), torch.full((3,), -1, dtype=torch.int64, device="cuda")
            gm._sync_stream()
            step(sol, norms, inert)
            torch.cuda.synchronize()
            assert inert[2].item() == 0 and inert[0].item() + inert[1].item() == n and torch.isfinite(norms).all()
            eager.append((sol, norms, inert))
        assert not torch.equal(_bits(eager[0][0]), _bits(eager[1][0]))
        sol, norms, inert = nan(n), nan(2), torch.full((3,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            gm._sync_stream()      # the handle follows torch's stream — inside the block that is the capturing one
            step(sol, norms, inert)
        gm._sync_stream()
        for i in (1, 0):
            load(i)
            sol.fill_(float("nan")); norms.fill_(float("nan")); inert.fill_(-1)
            g.replay()
            torch.cuda.synchronize()
            want = eager[i]
            assert torch.equal(_bits(sol), _bits(want[0])) and torch.equal(_bits(norms), _bits(want[1])) and torch.equal(inert, want[2]), (name, i)


def test_factor_async_refusals(built):
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib
    inert = torch.zeros(3, dtype=torch.int64, device="cuda")
    with solver("opf_7") as (gm, k):      # a border, mode 0
        assert gm._L.iem_kkt_factor_async(k, _p(inert)) == E_ARG and "mode 0" in gm._L.iem_last_error().decode()
    with solver("pandemic_300x7") as (gm, k):      # hub mode: the switch is a no-op, the asynchronous factorisation refused
        iemlib.check(gm._L.iem_kkt_set_border(k, 1))
        assert gm._L.iem_kkt_factor_async(k, _p(inert)) == E_ARG and "hub" in gm._L.iem_last_error().decode()


@pytest.mark.parametrize("name", ["farmer_5", "opf_7", "pandemic_100x7"])
def test_chain_kkt_with_the_border_on_the_device(name, built):
    """kkt_chain.ChainKKT(border="device"): the inertia of the default (torch) path, solutions against scipy with the tolerances
    of test_chain_kkt_on_gpu, and a matrix right-hand side column for column bitwise the single solve."""
    import torch
    from scipy.sparse.linalg import spsolve
    from infiniteexamodels.jl_amd.kkt import KKTSystem
    from infiniteexamodels.jl_amd.kkt_chain import ChainKKT
    from infiniteexamodels.jl_amd.model import ExaModel
    core, blob, om, pts = host(name)
    n = om.nvar + om.ncon
    gm = ExaModel(core, device=0, blob=blob)
    kkt = KKTSystem(gm)
    ck, ck0 = ChainKKT(kkt, border="device"), ChainKKT(kkt)
    assert ck.layout.ne > 0
    with pytest.raises(ValueError):
        ChainKKT(kkt, border="host")
    x, y, sigma, Kh, rhs = pts[0]
    xd, yd = torch.tensor(x, device="cuda"), torch.tensor(y, device="cuda")
    kkt.assemble(gm.hess_coord(xd, yd, obj_weight=1.0), gm.jac_coord(xd), torch.tensor(sigma, device="cuda"), DW, DC)
    assert ck.load().factor().inertia() == ck0.load().factor().inertia()
    rd = torch.tensor(rhs, device="cuda")
    sol = ck.solve(rd, refine=1).cpu().numpy()
    want = spsolve(Kh.tocsc(), rhs)
    resid = np.abs(Kh @ sol - rhs)
    assert resid.max() <= 1e-9 * max(1.0, np.abs(rhs).max()) or (resid / (abs(Kh) @ np.abs(sol) + np.abs(rhs))).max() <= 1e-12, name
    np.testing.assert_allclose(sol, want, rtol=1e-6, atol=1e-8 * max(1.0, np.abs(want).max()))
    R = torch.tensor(np.random.default_rng(21).standard_normal((n, 3)), device="cuda")
    X = ck.solve(R, refine=0)
    for j in range(3):
        assert torch.equal(_bits(X[:, j].contiguous()), _bits(ck.solve(R[:, j].contiguous(), refine=0))), (name, j)
    kkt.close(); gm.close()
