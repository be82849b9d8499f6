"""iem_kkt_solve_many / ChainKKT.solve with a 2-D right-hand side / sensitivity.parameter_steps on the MI355X.

Through the C-ABI object, assembled and factorised as tests/test_kkt_cabi.py::test_assemble_factor_solve_through_the_c_abi
does (sigma, 1e-2, 1e-6): every column meets that test's own two assertions against scipy after the same one host-formed
refinement step; the padding rows of a strided solution stay untouched; a column's bits depend neither on its place in
the batch nor on the other columns, and ARE the bits of iem_kkt_solve for that column; in place equals out of place; ten
repeats are identical; the argument errors.  Python: ChainKKT.solve column for column bitwise, and parameter_steps through
a real ChainKKT within the bound tests/test_gpu_param_sensitivity.py derives for the chain solve itself."""
import ctypes as C

import numpy as np
import pytest
from scipy.sparse.linalg import spsolve

import cases
from param_witness import WitnessA
from pyoracle import OracleModel
from test_gpu_param_sensitivity import CHAIN_BOUND
from test_kkt import host_kkt

pytestmark = pytest.mark.gpu
SENTINEL = -7.25e300
E_ARG = -4


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("name", ["quadrotor_100", "quadrotor_oc3_40", "farmer_5", "opf_7", "hovercraft", "kinetic_20", "quadrotor_1000",
                                  "pandemic_100x7", "pandemic_300x7"])      # (the last: hub mode, a loop of single solves)
def test_solve_many_through_the_c_abi(name, built):
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.model import ExaModel
    core = cases.build_core(name)
    blob = core.to_blob()
    om = OracleModel(blob)
    gm = ExaModel(core, device=0, blob=blob)
    L_ = gm._L
    k = C.c_void_p()
    iemlib.check(L_.iem_kkt_create(gm._h, 0, C.byref(k)))
    info = iemlib.KktInfo()
    iemlib.check(L_.iem_kkt_info(k, C.byref(info)))
    n = om.nvar + om.ncon
    assert info.n == n and bool(info.hubs) == (name == "pandemic_300x7")
    R = iemlib.kkt_many_width(info.nb, info.ne, info.nc)
    ld = n + 5
    f64 = dict(dtype=torch.float64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    try:
        # before a factorisation: refused with iem_kkt_solve's own words
        probe = torch.zeros(2, ld, **f64)
        assert L_.iem_kkt_solve(k, p(probe), p(probe)) == E_ARG
        words = L_.iem_last_error()
        assert L_.iem_kkt_solve_many(k, 2, p(probe), ld, p(probe), ld) == E_ARG and L_.iem_last_error() == words and b"no factorisation" in words

        rng = np.random.default_rng(3)
        x, y = cases.eval_point_for(name, om, 5)
        sigma = 0.5 + rng.random(om.nvar)
        xd, yd, sd = (torch.tensor(a, device="cuda") for a in (x, y, sigma))
        hv, jv = gm.hess_coord(xd, yd, obj_weight=1.0), gm.jac_coord(xd)
        gm._sync_stream()
        iemlib.check(L_.iem_kkt_assemble(k, p(hv), p(jv), p(sd), 1e-2, 1e-6))
        inertia = (C.c_int64 * 3)()
        iemlib.check(L_.iem_kkt_factor(k, inertia))
        Kh = host_kkt(om, x, y, sigma, 1e-2, 1e-6).tocsr()
        Kc = Kh.tocsc()

        def many(B, inplace=False):
            """Rows of B are the columns of the right-hand side (leading dimension ld, padding pre-filled)."""
            nk = B.shape[0]
            rd = torch.full((nk, ld), SENTINEL, **f64)
            rd[:, :n] = torch.tensor(B, device="cuda")
            if inplace:
                iemlib.check(L_.iem_kkt_solve_many(k, nk, p(rd), ld, p(rd), ld))
                out = rd
            else:
                before = rd.clone()
                out = torch.full((nk, ld), SENTINEL, **f64)
                iemlib.check(L_.iem_kkt_solve_many(k, nk, p(rd), ld, p(out), ld))
                assert torch.equal(rd, before)                                    # the right-hand side is only read
            assert bool((out[:, n:] == SENTINEL).all())                           # rows n .. ld of every column: neither read nor written
            return out[:, :n].cpu().numpy()

        def single(b):
            rd, sol = torch.tensor(b, device="cuda"), torch.empty(n, **f64)
            iemlib.check(L_.iem_kkt_solve(k, p(rd), p(sol)))
            return sol.cpu().numpy()

        B = rng.standard_normal((R + 3, n))
        singles = [single(B[u]) for u in range(R + 3)]
        for nk in (1, 3, R, R + 3):
            X = many(B[:nk])
            for u in range(nk):
                assert _same_bits(X[u], singles[u]), (name, nk, u)               # the single-column solve's bits
            res = B[:nk] - (Kh @ X.T).T                                           # one step of refinement, the residuals formed on the host
            X = X + many(res)
            for u in range(nk):
                rhs, xs = B[u], X[u]
                want = spsolve(Kc, rhs)
                resid = np.abs(Kh @ xs - rhs)
                assert resid.max() <= 1e-9 * max(1.0, np.abs(rhs).max()) or (resid / (abs(Kh) @ np.abs(xs) + np.abs(rhs))).max() <= 1e-12, (name, nk, u)
                np.testing.assert_allclose(xs, want, rtol=1e-6, atol=1e-8 * max(1.0, np.abs(want).max()))
            assert _same_bits(many(B[:nk], inplace=True), many(B[:nk]))          # in place = out of place
        # a column's bits do not depend on where it sits or on its neighbours
        a = many(B[[0, 1, 2]])
        b = many(B[[2, 0]])
        others = 10.0 * rng.standard_normal((R + 2, n))
        big = many(np.vstack([others[:R + 1], B[:1], others[R + 1:]]))             # b0 inside a batch of R + 3, behind the first full chunk
        assert big.shape[0] == R + 3
        assert _same_bits(a[0], b[1]) and _same_bits(a[2], b[0]) and _same_bits(a[0], big[R + 1]) and _same_bits(a[0], singles[0])
        zeros = many(np.vstack([B[:1], np.zeros((R + 2, n))]))
        assert _same_bits(zeros[0], a[0]) and not zeros[1:].any()
        first = many(B)
        for _ in range(10):
            assert _same_bits(many(B), first)
        # argument errors
        rd = torch.zeros(3 * ld + 8, **f64)
        out = torch.zeros(3 * ld + 8, **f64)
        assert L_.iem_kkt_solve_many(k, 3, p(rd), n - 1, p(out), ld) == E_ARG and b"leading dimension" in L_.iem_last_error()
        assert L_.iem_kkt_solve_many(k, 3, p(rd), ld, p(out), n - 1) == E_ARG
        assert L_.iem_kkt_solve_many(k, 3, p(rd), ld, C.c_void_p(rd.data_ptr() + 8 * 3), ld) == E_ARG and b"overlap" in L_.iem_last_error()
        assert L_.iem_kkt_solve_many(k, 3, p(rd), ld, p(rd), ld + 1) == E_ARG                       # the same array under another leading dimension
        assert L_.iem_kkt_solve_many(k, 0, p(rd), ld, p(out), ld) == E_ARG
        assert L_.iem_kkt_solve_many(k, 3, None, ld, p(out), ld) == E_ARG
    finally:
        iemlib.check(L_.iem_kkt_destroy(k))
        gm.close()


def _chain(name, seed=5):
    import torch
    from infiniteexamodels.jl_amd.kkt import KKTSystem
    from infiniteexamodels.jl_amd.kkt_chain import ChainKKT
    from infiniteexamodels.jl_amd.model import ExaModel
    core = cases.build_core(name)
    blob = core.to_blob()
    om = OracleModel(blob)
    gm = ExaModel(core, device=0, blob=blob)
    kkt = KKTSystem(gm)
    ck = ChainKKT(kkt)
    x, y = cases.eval_point_for(name, om, seed)
    rng = np.random.default_rng(3)
    sigma = 0.5 + rng.random(om.nvar)
    xd, yd = torch.tensor(x, device="cuda"), torch.tensor(y, device="cuda")
    kkt.assemble(gm.hess_coord(xd, yd, obj_weight=1.0), gm.jac_coord(xd), torch.tensor(sigma, device="cuda"), 1e-2, 1e-6)
    ck.load().factor()
    return core, om, gm, kkt, ck, x, y, sigma, xd, yd, rng


@pytest.mark.parametrize("name", ["quadrotor_1000", "pandemic_100x7"])
def test_chain_kkt_solve_takes_a_matrix(name, built):
    import torch
    core, om, gm, kkt, ck, x, y, sigma, xd, yd, rng = _chain(name)
    try:
        n = om.nvar + om.ncon
        wide = torch.tensor(rng.standard_normal((n, 10)), device="cuda")
        rhs = wide[:, ::2]                                                         # five columns, none of them contiguous
        assert not rhs.is_contiguous() and rhs.shape == (n, 5)
        got = ck.solve(rhs, refine=1)
        assert tuple(got.shape) == (n, 5)
        for u in range(5):
            one = ck.solve(rhs[:, u].contiguous(), refine=1)
            assert one.shape == (n,)
            assert _same_bits(got[:, u].cpu().numpy(), one.cpu().numpy()), (name, u)
        auto = ck.solve(rhs, refine="auto")
        for u in range(5):
            assert _same_bits(auto[:, u].cpu().numpy(), ck.solve(rhs[:, u].contiguous(), refine="auto").cpu().numpy()), (name, u)
        assert _same_bits(ck.solve(rhs.contiguous(), refine=0).cpu().numpy(), ck.solve(rhs, refine=0).cpu().numpy())
    finally:
        kkt.close(); gm.close()


def test_parameter_steps_through_the_chain_solver(built):
    """Four random directions at once through a real ChainKKT on the quadrotor at 1 000 supports, set up as
    tests/test_gpu_param_sensitivity.py::test_parameter_step_through_the_chain_solver: K from the oracle, the right-hand sides
    from witness A, scipy's sparse LU; the bound is that test's CHAIN_BOUND (3.346e-12: ten times what the untouched
    single-column chain solve reaches against scipy at this size)."""
    import torch
    from infiniteexamodels.jl_amd.sensitivity import parameter_steps
    core, om, gm, kkt, ck, x, y, sigma, xd, yd, rng = _chain("quadrotor_1000")
    try:
        nk = 4
        dth = 0.1 * rng.standard_normal((om.npar, nk))
        dX, dY = parameter_steps(gm, ck, xd, yd, torch.tensor(dth, device="cuda"))
        assert tuple(dX.shape) == (om.nvar, nk) and tuple(dY.shape) == (om.ncon, nk)
        A = WitnessA(core)
        Kc = host_kkt(om, x, y, sigma, 1e-2, 1e-6).tocsc()
        for u in range(nk):
            d = np.ascontiguousarray(dth[:, u])
            rhs = -np.concatenate([A.hpprod(x, y, d, 1.0), A.jpprod(x, d)])
            want = spsolve(Kc, rhs)
            got = np.concatenate([dX[:, u].cpu().numpy(), dY[:, u].cpu().numpy()])
            err = np.abs(got - want).max() / max(1.0, np.abs(want).max())
            print(f"parameter_steps column {u} through ChainKKT: {err:.3e} (bound {CHAIN_BOUND:.3e}), max |step| {np.abs(want).max():.3e}")
            assert np.abs(want).max() > 0 and err <= CHAIN_BOUND
    finally:
        kkt.close(); gm.close()
