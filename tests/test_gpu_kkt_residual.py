"""iem_kkt_residual and iem_kkt_solve_refined on the MI355X: the matrix-free residual rhs − K·sol against scipy on the oracle's KKT
matrix, its norm bitwise max|r|, the refined solve bitwise the hand loop of iem_kkt_solve / iem_kkt_residual / a vector add, a graph
capture, and what one step of refinement buys against a residual formed in float64 on the host."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import cases
from pyoracle import OracleModel
from test_kkt import host_kkt

pytestmark = pytest.mark.gpu
MODELS = ["quadrotor_100", "quadrotor_1000", "pandemic_20x3"]      # 1-D chains (one / several workgroups of the operator) and a 2-D grid as lanes with a border
DW, DC, SIGMA_W = 1e-2, 1e-6, 0.9
EPS = 2.0 ** -52


def _bits(t):
    import torch
    return t.view(torch.int64)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


_host = {}


def host(name):
    """(core, blob, oracle, x, y, sigma, K of scipy, rhs): built once per model, shared by the tests and left unchanged"""
    if name not in _host:
        core = cases.build_core(name)
        blob = core.to_blob()
        om = OracleModel(blob)
        x, y = cases.eval_point_for(name, om, 5)
        rng = np.random.default_rng(3)
        sigma = 0.5 + rng.random(om.nvar)
        K = host_kkt(om, x, y, sigma, DW, DC, SIGMA_W)
        _host[name] = (core, blob, om, x, y, sigma, K, rng.standard_normal(om.nvar + om.ncon))
    return _host[name]


@contextlib.contextmanager
def system(name, factor=True):
    """the model handle, the solver object assembled and factorised at the point of host(name), and the device vectors"""
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.model import ExaModel
    core, blob, om, x, y, sigma, K, rhs = host(name)
    gm = ExaModel(core, device=0, blob=blob)
    k = C.c_void_p()
    iemlib.check(gm._L.iem_kkt_create(gm._h, 0, C.byref(k)))
    try:
        xd, yd, sd, rd = (torch.tensor(a, device="cuda") for a in (x, y, sigma, rhs))
        if factor:
            hv, jv = gm.hess_coord(xd, yd, obj_weight=SIGMA_W), gm.jac_coord(xd)
            gm._sync_stream()
            iemlib.check(gm._L.iem_kkt_assemble(k, _p(hv), _p(jv), _p(sd), DW, DC))
            inertia = (C.c_int64 * 3)()
            iemlib.check(gm._L.iem_kkt_factor(k, inertia))
            assert inertia[2] == 0 and inertia[0] + inertia[1] == om.nvar + om.ncon, tuple(inertia)      # (W at a random y is indefinite: more than ncon negative pivots, none doubtful)
        gm._sync_stream()
        yield gm, k, xd, yd, sd, rd
    finally:
        iemlib.check(gm._L.iem_kkt_destroy(k))
        gm.close()


def residual(gm, k, xd, yd, sd, rhs, sol, r, norm, dw=DW, dc=DC):
    from infiniteexamodels.jl_amd import lib as iemlib
    iemlib.check(gm._L.iem_kkt_residual(k, _p(xd), _p(yd), SIGMA_W, _p(sd), dw, dc, _p(rhs), _p(sol), _p(r), _p(norm)))
    return r


def solve(gm, k, rhs, sol):
    from infiniteexamodels.jl_amd import lib as iemlib
    iemlib.check(gm._L.iem_kkt_solve(k, _p(rhs), _p(sol)))
    return sol


def refined(gm, k, xd, yd, sd, rhs, sol, steps, norms):
    from infiniteexamodels.jl_amd import lib as iemlib
    iemlib.check(gm._L.iem_kkt_solve_refined(k, _p(xd), _p(yd), SIGMA_W, _p(sd), DW, DC, _p(rhs), _p(sol), steps, _p(norms)))
    return sol


def nan(n):
    import torch
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


@pytest.mark.parametrize("name", MODELS)
def test_residual_and_its_norm(name, built):
    """r against the float64 scipy residual to 1e-10·(‖|K||sol|‖∞ + ‖rhs‖∞), d_norm bitwise max|r| (torch on the returned r) — for
    a random sol, for the solution of the system, without sigma, in place on rhs, and without a norm.  No factorisation needed."""
    import torch
    core, blob, om, x, y, sigma, K, rhs = host(name)
    n = om.nvar + om.ncon
    with system(name, factor=False) as (gm, k, xd, yd, sd, rd):
        from scipy.sparse.linalg import spsolve
        for which, sol in (("random", np.random.default_rng(8).standard_normal(n)), ("solution", spsolve(K.tocsc(), rhs))):
            sold, r, norm = torch.tensor(sol, device="cuda"), nan(n), nan(1)
            residual(gm, k, xd, yd, sd, rd, sold, r, norm)
            want = rhs - K @ sol
            bound = 1e-10 * (np.abs(abs(K) @ np.abs(sol)).max() + np.abs(rhs).max())
            err = np.abs(r.cpu().numpy() - want).max()
            print(name, which, "err", err, "bound", bound, "norm", float(norm.item()))
            assert err <= bound
            assert torch.equal(_bits(norm), _bits(r.abs().max().reshape(1)))
        # sigma = NULL, other shifts
        K0 = host_kkt(om, x, y, np.zeros(om.nvar), 0.3, 0.0, SIGMA_W)
        r0 = residual(gm, k, xd, yd, None, rd, sold, nan(n), None, dw=0.3, dc=0.0)
        assert np.abs(r0.cpu().numpy() - (rhs - K0 @ sol)).max() <= 1e-10 * (np.abs(abs(K0) @ np.abs(sol)).max() + np.abs(rhs).max())
        # in place on a copy of rhs, bitwise the same r
        inplace = rd.clone()
        residual(gm, k, xd, yd, sd, inplace, sold, inplace, None)
        assert torch.equal(_bits(inplace), _bits(r))
        # a NaN in sol is a NaN norm
        bad = sold.clone(); bad[n // 2] = float("nan")
        residual(gm, k, xd, yd, sd, rd, bad, nan(n), norm)
        assert torch.isnan(norm).all()
        # r on sol is refused
        rc = gm._L.iem_kkt_residual(k, _p(xd), _p(yd), SIGMA_W, _p(sd), DW, DC, _p(rd), _p(sold), _p(sold), None)
        assert rc == -4 and "overlap" in gm._L.iem_last_error().decode()


@pytest.mark.parametrize("name", MODELS)
def test_refined_solve_is_the_hand_loop(name, built):
    """steps = 2: sol and d_norms bitwise the loop  solve / residual / torch add;  steps = 0: bitwise iem_kkt_solve, one norm."""
    import torch
    core, blob, om, x, y, sigma, K, rhs = host(name)
    n = om.nvar + om.ncon
    with system(name) as (gm, k, xd, yd, sd, rd):
        sol = solve(gm, k, rd, nan(n))
        sol0 = sol.clone()
        norms_hand = []
        for _ in range(2):
            r, nm = nan(n), nan(1)
            residual(gm, k, xd, yd, sd, rd, sol, r, nm)
            norms_hand.append(nm)
            sol = sol + solve(gm, k, r, nan(n))
        nm = nan(1)
        residual(gm, k, xd, yd, sd, rd, sol, nan(n), nm)
        norms_hand = torch.cat(norms_hand + [nm])
        got, norms = nan(n), nan(3)
        refined(gm, k, xd, yd, sd, rd, got, 2, norms)
        print(name, "norms", norms.tolist())
        assert torch.equal(_bits(got), _bits(sol)) and torch.equal(_bits(norms), _bits(norms_hand))
        assert torch.isfinite(norms).all()
        # without norms: the same solution
        assert torch.equal(_bits(refined(gm, k, xd, yd, sd, rd, nan(n), 2, None)), _bits(sol))
        # steps = 0
        z, n0 = nan(n), nan(1)
        refined(gm, k, xd, yd, sd, rd, z, 0, n0)
        assert torch.equal(_bits(z), _bits(sol0)) and torch.equal(_bits(n0), _bits(norms_hand[:1]))
        assert torch.equal(_bits(refined(gm, k, xd, yd, sd, rd, nan(n), 0, None)), _bits(sol0))
        # refusals
        L = gm._L
        assert L.iem_kkt_solve_refined(k, _p(xd), _p(yd), SIGMA_W, _p(sd), DW, DC, _p(rd), _p(rd), 1, None) == -4
        assert L.iem_kkt_solve_refined(k, _p(xd), _p(yd), SIGMA_W, _p(sd), DW, DC, _p(rd), _p(z), -1, None) == -4


def test_refined_solve_needs_factors(built):
    import torch
    om = host("quadrotor_100")[2]
    n = om.nvar + om.ncon
    with system("quadrotor_100", factor=False) as (gm, k, xd, yd, sd, rd):
        rc = gm._L.iem_kkt_solve_refined(k, _p(xd), _p(yd), SIGMA_W, _p(sd), DW, DC, _p(rd), _p(nan(n)), 1, None)
        assert rc == -4 and "factorisation" in gm._L.iem_last_error().decode()


def test_refined_solve_is_capturable(built):
    """quadrotor_1000 (no border: nothing of the solve runs on the host): one direct call does the set-up, then one capture of
    iem_kkt_solve_refined(steps = 1) with norms, three replays, each bitwise the direct call."""
    import torch
    name = "quadrotor_1000"
    om = host(name)[2]
    n = om.nvar + om.ncon
    with system(name) as (gm, k, xd, yd, sd, rd):
        sol0, norms0 = nan(n), nan(2)
        refined(gm, k, xd, yd, sd, rd, sol0, 1, norms0)
        sol, norms = nan(n), nan(2)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            gm._sync_stream()      # the handle follows torch's stream — inside the block that is the capturing one
            refined(gm, k, xd, yd, sd, rd, sol, 1, norms)
        gm._sync_stream()
        for _ in range(3):
            sol.fill_(float("nan")); norms.fill_(float("nan"))
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(_bits(sol), _bits(sol0)) and torch.equal(_bits(norms), _bits(norms0))


@pytest.mark.parametrize("name", MODELS)
def test_what_refinement_buys(name, built):
    """The scipy residual of steps = 1 against that of the host-formed step x1 = x0 + solve(rhs − K_scipy·x0), both solves through
    iem_kkt_solve: the two differ only in the rounding of the residual, so the refined one may be at most 4 x the host-formed one
    plus (nvar + ncon)·2⁻⁵²·(‖|K||x1|‖∞ + ‖rhs‖∞), and it must be smaller than the unrefined residual whenever that exceeds the
    floor.  Measured on the MI355X, unrefined / host-formed / refined:
        quadrotor_100   1.9e-12 / 6.9e-14 / 6.5e-14     quadrotor_1000   7.1e-10 / 3.3e-12 / 2.9e-12     pandemic_20x3   5.0e-5 / 3.0e-10 / 2.5e-10"""
    import torch
    core, blob, om, x, y, sigma, K, rhs = host(name)
    n = om.nvar + om.ncon
    with system(name) as (gm, k, xd, yd, sd, rd):
        x0 = solve(gm, k, rd, nan(n)).cpu().numpy()
        r_host = torch.tensor(rhs - K @ x0, device="cuda")
        x1 = x0 + solve(gm, k, r_host, nan(n)).cpu().numpy()
        xr = refined(gm, k, xd, yd, sd, rd, nan(n), 1, None).cpu().numpy()
        res = lambda v: float(np.abs(rhs - K @ v).max())
        unrefined, host_formed, device = res(x0), res(x1), res(xr)
        floor = n * EPS * (np.abs(abs(K) @ np.abs(x1)).max() + np.abs(rhs).max())
        print(name, f"unrefined {unrefined:.3e} host-formed {host_formed:.3e} refined {device:.3e} floor {floor:.3e}")
        assert device <= 4.0 * host_formed + floor
        if unrefined > floor:
            assert device < unrefined


@pytest.mark.parametrize("name", ["quadrotor_100", "pandemic_20x3"])
def test_chain_kkt_refines_through_the_operator(name, built):
    """The Python layer: MatrixFreeKKT.matvec on the device against the CSR product (ChainKKT._matvec) and scipy to the suite's
    1e-10, and ChainKKT.solve(refine = 1, operator = op) against the default (CSR) refinement — the same solves, residuals that
    differ only in their rounding: at most 4 x the CSR-refined scipy residual plus the floor of the test above; one column or
    several."""
    import torch
    from infiniteexamodels.jl_amd.kkt import KKTSystem
    from infiniteexamodels.jl_amd.kkt_chain import ChainKKT, MatrixFreeKKT
    from infiniteexamodels.jl_amd.model import ExaModel
    core, blob, om, x, y, sigma, K, rhs = host(name)
    n = om.nvar + om.ncon
    gm = ExaModel(core, device=0, blob=blob)
    kk = KKTSystem(gm)
    try:
        xd, yd, sd, rd = (torch.tensor(a, device="cuda") for a in (x, y, sigma, rhs))
        kk.assemble(gm.hess_coord(xd, yd, obj_weight=SIGMA_W), gm.jac_coord(xd), sd, DW, DC)
        ck = ChainKKT(kk).load().factor()
        op = MatrixFreeKKT(gm, xd, yd, SIGMA_W, sd, DW, DC)
        z = np.random.default_rng(12).standard_normal(n)
        zd = torch.tensor(z, device="cuda")
        want = K @ z
        scale = max(1.0, np.abs(want).max())
        assert np.abs(op.matvec(zd).cpu().numpy() - want).max() <= 1e-10 * scale
        assert float((op.matvec(zd) - ck._matvec(zd)).abs().max().item()) <= 1e-10 * scale
        assert np.abs(op.residual(rd, zd).cpu().numpy() - (rhs - want)).max() <= 1e-10 * (scale + np.abs(rhs).max())
        res = lambda v: float(np.abs(rhs - K @ v).max())
        x_csr, x_op = ck.solve(rd, refine=1).cpu().numpy(), ck.solve(rd, refine=1, operator=op).cpu().numpy()
        floor = n * EPS * (np.abs(abs(K) @ np.abs(x_csr)).max() + np.abs(rhs).max())
        print(name, f"unrefined {res(ck.solve(rd, refine=0).cpu().numpy()):.3e} csr-refined {res(x_csr):.3e} operator-refined {res(x_op):.3e} floor {floor:.3e}")
        assert res(x_op) <= 4.0 * res(x_csr) + floor
        two = torch.stack([rd, 2.0 * rd + 1.0], 1)
        X = ck.solve(two, refine=1, operator=op)
        assert torch.equal(_bits(X[:, 0].contiguous()), _bits(ck.solve(rd, refine=1, operator=op)))
        assert torch.equal(_bits(X[:, 1].contiguous()), _bits(ck.solve(two[:, 1].contiguous(), refine=1, operator=op)))
    finally:
        kk.close()
        gm.close()
