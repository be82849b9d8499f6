"""iem_kkt_assemble_diag / iem_kkt_residual_diag / iem_kkt_solve_refined_diag and kkt_chain.KKTObject on the MI355X: the KKT object
with a per-row diagonal −diag(dcon + delta_c) in its constraint block, and the residual / refined solve over several columns.

What is derivable is checked BITWISE (no tolerance): the scalar cases against iem_kkt_assemble / iem_kkt_residual /
iem_kkt_solve_refined, a column of a multi-column call against the call on that column alone, the refined solve against its hand
loop, r against tests/kkt_diag_reference.py on iem_kktprod's output, the norms against max|r|.  Values: the inertia against the
eigenvalues (or, in hub mode, kkt_chain.HubChainKKT), the residual against scipy, one step of refinement against the criterion of
tests/test_kkt_cabi.py.

Modes of the object: quadrotor_100 and pandemic_20x3 are 1-D chains without a border (iem_kkt_set_border is a no-op for them: the
two modes of pandemic_20x3 run the same code), opf_7 has a dense border of 52 and pandemic_100x7 is lanes with a dense border of
100 — those two are where modes 0 and 1 differ —, pandemic_300x7 keeps its border as hubs."""
import contextlib
import ctypes as C
import types

import numpy as np
import pytest

import kkt_diag_reference as dref
from kkt_diag_reference import DC, DW

pytestmark = pytest.mark.gpu
MODELS = ["quadrotor_100", "pandemic_20x3", "opf_7", "pandemic_300x7"]
CASES = [("quadrotor_100", 0), ("pandemic_20x3", 0), ("pandemic_20x3", 1), ("opf_7", 0), ("opf_7", 1), ("pandemic_100x7", 0), ("pandemic_100x7", 1), ("pandemic_300x7", 0)]
NRHS = (1, 3, 9)      # 9: across a slab seam (8), and a chunk tail of the multi-column kernels (widths 2 / 4)
PAD = 5


def _bits(t):
    import torch
    return t.contiguous().view(torch.int64)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def nan(*shape):
    import torch
    return torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")


def padded(a):
    """rows of `a` (K, n) as the columns of a NaN-poisoned buffer with ld = n + PAD"""
    buf = nan(a.shape[0], a.shape[1] + PAD)
    buf[:, :a.shape[1]] = a
    return buf


def padding_untouched(buf, n):
    import torch
    return bool(torch.isnan(buf[:, n:]).all())


@contextlib.contextmanager
def system(name, mode=0):
    """the model handle, the raw solver object in border mode `mode`, and the device vectors of dref.host_system(name)"""
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.model import ExaModel
    h = dref.host_system(name)
    gm = ExaModel(h["core"], device=0, blob=h["blob"])
    k = C.c_void_p()
    iemlib.check(gm._L.iem_kkt_create(gm._h, 0, C.byref(k)))
    try:
        S = types.SimpleNamespace(gm=gm, L=gm._L, k=k, h=h, n=h["om"].nvar + h["om"].ncon, nvar=h["om"].nvar, ncon=h["om"].ncon, check=iemlib.check)
        S.xd, S.yd, S.sd, S.dd = (torch.tensor(h[a], device="cuda") for a in ("x", "y", "sigma", "dcon"))
        S.hv, S.jv = gm.hess_coord(S.xd, S.yd, obj_weight=1.0), gm.jac_coord(S.xd)
        S.B = torch.tensor(np.random.default_rng(11).standard_normal((max(NRHS), S.n)), device="cuda")
        S.B[0] = torch.tensor(h["rhs"], device="cuda")
        gm._sync_stream()
        S.check(S.L.iem_kkt_set_border(k, mode))
        yield S
    finally:
        iemlib.check(gm._L.iem_kkt_destroy(k))
        gm.close()


def assemble_diag(S, dcon, dc=DC):
    S.gm._sync_stream()
    S.check(S.L.iem_kkt_assemble_diag(S.k, _p(S.hv), _p(S.jv), _p(S.sd), _p(dcon), DW, dc))


def factor(S):
    inertia = (C.c_int64 * 3)()
    S.check(S.L.iem_kkt_factor(S.k, inertia))
    return tuple(inertia)


def solve(S, rhs):
    sol = nan(S.n)
    S.check(S.L.iem_kkt_solve(S.k, _p(rhs), _p(sol)))
    return sol


def residual_diag(S, dcon, rhs, sol, norms=True, r=None, dc=DC):
    """rhs, sol: padded (K, ld) buffers; returns (r buffer, norms)"""
    K, ld = rhs.shape
    r = nan(K, ld) if r is None else r
    nm = nan(K) if norms else None
    S.check(S.L.iem_kkt_residual_diag(S.k, _p(S.xd), _p(S.yd), 1.0, _p(S.sd), _p(dcon), DW, dc, K, _p(rhs), ld, _p(sol), sol.shape[1], _p(r), r.shape[1], _p(nm)))
    return r, nm


def refined_diag(S, dcon, rhs, steps, norms=True, dc=DC):
    K, ld = rhs.shape
    sol = nan(K, ld)
    nm = nan(steps + 1, K) if norms else None
    S.check(S.L.iem_kkt_solve_refined_diag(S.k, _p(S.xd), _p(S.yd), 1.0, _p(S.sd), _p(dcon), DW, dc, K, _p(rhs), ld, _p(sol), ld, steps, _p(nm)))
    return sol, nm


def solve_many(S, rhs):
    sol = nan(*rhs.shape)
    S.check(S.L.iem_kkt_solve_many(S.k, rhs.shape[0], _p(rhs), rhs.shape[1], _p(sol), sol.shape[1]))
    return sol


@pytest.mark.parametrize("name,mode", CASES)
def test_assemble_identities_and_inertia(name, mode, built):
    """dcon = NULL and dcon ≡ d with delta_c = 0 give the inertia and the solution bits of iem_kkt_assemble (−(d + 0.0) = −d); with the
    vector of the CPU test the pivot signs are the inertia of K (eigenvalues for n <= 4000; HubChainKKT fed by KKTSystem.assemble
    with the tensor as witness in hub mode), and one refined solve meets the criterion."""
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib
    with system(name, mode) as S:
        S.check(S.L.iem_kkt_assemble(S.k, _p(S.hv), _p(S.jv), _p(S.sd), DW, DC))
        want = factor(S)
        sol0 = solve(S, S.B[0])
        assert want[2] == 0 and want[0] + want[1] == S.n
        for dcon, dc in ((None, DC), (torch.full((S.ncon,), DC, dtype=torch.float64, device="cuda"), 0.0)):
            assemble_diag(S, dcon, dc)
            rc = S.L.iem_kkt_solve(S.k, _p(S.B[0]), _p(nan(S.n)))
            assert rc == -4 and "factorisation" in S.L.iem_last_error().decode()      # assembling invalidates the factors
            assert factor(S) == want
            assert torch.equal(_bits(solve(S, S.B[0])), _bits(sol0))
        assemble_diag(S, S.dd)
        inertia = factor(S)
        print(name, mode, "inertia", inertia, "eigenvalues", S.h["neg"])
        assert inertia[2] == 0 and inertia[0] + inertia[1] == S.n and inertia[1] >= S.ncon
        if S.h["neg"] is not None:
            assert inertia[1] == S.h["neg"]
        info = iemlib.KktInfo()
        S.check(S.L.iem_kkt_info(S.k, C.byref(info)))
        assert bool(info.hubs) == (name == "pandemic_300x7")
        if info.hubs:
            from infiniteexamodels.jl_amd.kkt import KKTSystem
            from infiniteexamodels.jl_amd.kkt_chain import HubChainKKT
            kk = KKTSystem(S.gm)
            kk.assemble(S.hv, S.jv, S.sd, DW, S.dd + DC)
            assert inertia == HubChainKKT(kk).load().factor().inertia()
            kk.close()
            S.gm._sync_stream()
        sol, _ = refined_diag(S, S.dd, padded(S.B[:1]), 1, norms=False)
        ok, resid, comp = dref.residual_ok(S.h["K"], sol[0, :S.n].cpu().numpy(), S.B[0].cpu().numpy())
        print(name, mode, "residual after one step", resid, "componentwise", comp)
        assert ok


@pytest.mark.parametrize("name", MODELS)
def test_residual_identities_and_values(name, built):
    """(the factors are not touched: no mode, no factorisation)"""
    import torch
    from test_kkt import host_kkt
    with system(name) as S:
        n, nvar = S.n, S.nvar
        sol9 = torch.tensor(np.random.default_rng(8).standard_normal((max(NRHS), n)), device="cuda")
        rhs, sol = padded(S.B), padded(sol9)
        # iem_kktprod's output per column, for the reference's expression
        P = torch.stack([torch.cat(S.gm.kktprod(S.xd, S.yd, sol9[u, :nvar].contiguous(), sol9[u, nvar:].contiguous(), obj_weight=1.0)) for u in range(sol9.shape[0])]).cpu().numpy()
        S.gm._sync_stream()
        for dcon, K in ((None, host_kkt(S.h["om"], S.h["x"], S.h["y"], S.h["sigma"], DW, DC)), (S.dd, S.h["K"])):
            single = [residual_diag(S, dcon, rhs[u:u + 1], sol[u:u + 1]) for u in range(rhs.shape[0])]
            for nrhs in NRHS:
                r, nm = residual_diag(S, dcon, rhs[:nrhs], sol[:nrhs])
                assert padding_untouched(r, n)
                for u in range(nrhs):      # a column carries the bits of the call on that column alone
                    assert torch.equal(_bits(r[u, :n]), _bits(single[u][0][0, :n])) and torch.equal(_bits(nm[u:u + 1]), _bits(single[u][1]))
                assert torch.equal(_bits(nm), _bits(r[:, :n].abs().max(dim=1).values))
                want, want_nm = dref.residual_dm(P[:nrhs], S.B[:nrhs].cpu().numpy(), sol9[:nrhs].cpu().numpy(), S.h["sigma"], None if dcon is None else S.h["dcon"], DW, DC, nvar)
                assert np.array_equal(r[:, :n].cpu().numpy().view(np.int64), want.view(np.int64))
                assert np.array_equal(nm.cpu().numpy().view(np.int64), want_nm.view(np.int64))
                assert torch.equal(_bits(residual_diag(S, dcon, rhs[:nrhs], sol[:nrhs], norms=False)[0][:, :n]), _bits(r[:, :n]))
            got, b, x = r[:, :n].cpu().numpy(), S.B.cpu().numpy(), sol9.cpu().numpy()
            for u in range(max(NRHS)):      # against scipy
                bound = 1e-10 * (np.abs(abs(K) @ np.abs(x[u])).max() + np.abs(b[u]).max())
                err = np.abs(got[u] - (b[u] - K @ x[u])).max()
                assert err <= bound, (name, u, err, bound)
            print(name, "dcon" if dcon is not None else "scalar", "column 0: err", np.abs(got[0] - (b[0] - K @ x[0])).max(), "norm", float(nm[0]))
        # nrhs = 1 without dcon: the bits of iem_kkt_residual
        r1, n1 = nan(n), nan(1)
        S.check(S.L.iem_kkt_residual(S.k, _p(S.xd), _p(S.yd), 1.0, _p(S.sd), DW, DC, _p(S.B[0]), _p(sol9[0]), _p(r1), _p(n1)))
        rd, nd = residual_diag(S, None, rhs[:1], sol[:1])
        assert torch.equal(_bits(rd[0, :n]), _bits(r1)) and torch.equal(_bits(nd), _bits(n1))
        # in place on a copy of rhs: the same bits
        r9, _ = residual_diag(S, S.dd, rhs, sol)
        inplace = rhs.clone()
        residual_diag(S, S.dd, inplace, sol, r=inplace)
        assert torch.equal(_bits(inplace[:, :n]), _bits(r9[:, :n])) and padding_untouched(inplace, n)
        # a NaN entry of dcon is not inspected: it reaches the residual of every column whose sol is non-zero on that row
        bad = S.dd.clone(); bad[S.ncon // 2] = float("nan")
        assert bool((sol9[:, nvar + S.ncon // 2] != 0).all())
        rb, nb_ = residual_diag(S, bad, rhs, sol)
        assert bool(torch.isnan(nb_).all()) and int(torch.isnan(rb[:, :n]).sum().item()) == rhs.shape[0]


@pytest.mark.parametrize("name,mode", CASES)
def test_refined_solve_identities_and_values(name, mode, built):
    import torch
    with system(name, mode) as S:
        n = S.n
        rhs = padded(S.B)
        # scalar matrices, nrhs = 1, no dcon, steps = 2: the bits of iem_kkt_solve_refined
        S.check(S.L.iem_kkt_assemble(S.k, _p(S.hv), _p(S.jv), _p(S.sd), DW, DC))
        factor(S)
        want, want_nm = nan(n), nan(3)
        S.check(S.L.iem_kkt_solve_refined(S.k, _p(S.xd), _p(S.yd), 1.0, _p(S.sd), DW, DC, _p(S.B[0]), _p(want), 2, _p(want_nm)))
        got, got_nm = refined_diag(S, None, rhs[:1], 2)
        assert torch.equal(_bits(got[0, :n]), _bits(want)) and torch.equal(_bits(got_nm[:, 0]), _bits(want_nm)) and padding_untouched(got, n)
        # the per-row diagonal
        assemble_diag(S, S.dd)
        factor(S)
        single = [refined_diag(S, S.dd, rhs[u:u + 1], 2) for u in range(rhs.shape[0])]
        for nrhs in NRHS[1:]:
            sol, nm = refined_diag(S, S.dd, rhs[:nrhs], 2)
            assert padding_untouched(sol, n) and bool(torch.isfinite(nm).all())
            for u in range(nrhs):
                assert torch.equal(_bits(sol[u, :n]), _bits(single[u][0][0, :n])) and torch.equal(_bits(nm[:, u]), _bits(single[u][1][:, 0])), (nrhs, u)
            assert torch.equal(_bits(refined_diag(S, S.dd, rhs[:nrhs], 2, norms=False)[0][:, :n]), _bits(sol[:, :n]))
        # ... is the hand loop: iem_kkt_solve_many, iem_kkt_residual_diag, iem_kkt_solve_many, torch's add
        X = solve_many(S, rhs)
        hand_nm = []
        for _ in range(2):
            r, nrm = residual_diag(S, S.dd, rhs, X)
            hand_nm.append(nrm)
            dX = solve_many(S, r)
            X[:, :n] = X[:, :n] + dX[:, :n]
        hand_nm.append(residual_diag(S, S.dd, rhs, X)[1])
        assert torch.equal(_bits(sol[:, :n]), _bits(X[:, :n])) and torch.equal(_bits(nm), _bits(torch.stack(hand_nm)))
        print(name, mode, "norms of column 0 in front of step 0, 1 and behind:", nm[:, 0].tolist())
        # steps = 0 is iem_kkt_solve_many and one row of norms
        s0, n0 = refined_diag(S, S.dd, rhs[:3], 0)
        assert torch.equal(_bits(s0[:, :n]), _bits(solve_many(S, rhs[:3])[:, :n])) and n0.shape == (1, 3) and bool(torch.isfinite(n0).all())
        # steps = 1 meets the criterion on every column; ten identical repetitions
        first, first_nm = refined_diag(S, S.dd, rhs, 1)
        b, x = S.B.cpu().numpy(), first[:, :n].cpu().numpy()
        for u in range(rhs.shape[0]):
            ok, resid, comp = dref.residual_ok(S.h["K"], x[u], b[u])
            assert ok, (name, mode, u, resid, comp)
        for _ in range(10):
            again, again_nm = refined_diag(S, S.dd, rhs, 1)
            assert torch.equal(_bits(again), _bits(first)) and torch.equal(_bits(again_nm), _bits(first_nm))


@pytest.mark.parametrize("name", ["pandemic_20x3", "opf_7"])
def test_assemble_factor_refined_solve_in_one_graph(name, built):
    """border mode 1 (opf_7: the border's LDL' and its solves on the device; pandemic_20x3 has no border): iem_kkt_assemble_diag +
    iem_kkt_factor_async + iem_kkt_solve_refined_diag(nrhs = 3, steps = 1) captured once, replayed with other dcon values in the
    same buffer — each replay bitwise the direct calls with those values."""
    import torch
    with system(name, 1) as S:
        n = S.n
        rhs = padded(S.B[:3])
        dbuf = S.dd.clone()
        inertia = torch.zeros(3, dtype=torch.int64, device="cuda")
        sol, nm = nan(3, n + PAD), nan(2, 3)

        def sequence():
            S.gm._sync_stream()
            S.check(S.L.iem_kkt_assemble_diag(S.k, _p(S.hv), _p(S.jv), _p(S.sd), _p(dbuf), DW, DC))
            S.check(S.L.iem_kkt_factor_async(S.k, _p(inertia)))
            S.check(S.L.iem_kkt_solve_refined_diag(S.k, _p(S.xd), _p(S.yd), 1.0, _p(S.sd), _p(dbuf), DW, DC, 3, _p(rhs), n + PAD, _p(sol), n + PAD, 1, _p(nm)))
        other = torch.flip(S.dd, dims=(0,)) * 3.0 + 1e-3
        direct = {}
        for key, vals in (("other", other), ("first", S.dd)):      # the direct calls (the first one does the set-up)
            dbuf.copy_(vals)
            sequence()
            torch.cuda.synchronize()
            direct[key] = (sol.clone(), nm.clone(), inertia.clone())
        assert not torch.equal(_bits(direct["first"][0][:, :n]), _bits(direct["other"][0][:, :n]))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            sequence()
        S.gm._sync_stream()
        for key, vals in (("first", S.dd), ("other", other), ("first", S.dd)):
            dbuf.copy_(vals)
            sol.fill_(float("nan")); nm.fill_(float("nan")); inertia.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(_bits(sol[:, :n]), _bits(direct[key][0][:, :n])) and torch.equal(_bits(nm), _bits(direct[key][1])) and torch.equal(inertia, direct[key][2])
            assert padding_untouched(sol, n) and int(inertia[2]) == 0 and int(inertia[0] + inertia[1]) == n


def test_refusals(built):
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.kkt_chain import KKTObject
    from infiniteexamodels.jl_amd.model import ExaModel
    with system("quadrotor_100") as S:
        n, L = S.n, S.L
        rhs, sol = padded(S.B[:3]), padded(S.B[:3] * 0.5)
        ld = n + PAD
        common = (S.k, _p(S.xd), _p(S.yd), 1.0, _p(S.sd), _p(S.dd), DW, DC)
        err = lambda: L.iem_last_error().decode()
        res = lambda nrhs, b, ldb, x, ldx, r, ldr, nm=None: L.iem_kkt_residual_diag(*common, nrhs, _p(b), ldb, _p(x), ldx, _p(r), ldr, _p(nm))
        out = nan(3, ld)
        assert res(3, rhs, ld, sol, ld, sol, ld) == -4 and "overlap" in err()                       # r on sol
        assert res(2, rhs, 2 * ld, sol, ld, rhs[1:], 2 * ld) == -4 and "overlap" in err()           # r's columns between those of rhs
        assert res(3, rhs, ld, sol, ld, out, ld, sol[0, :3]) == -4 and "overlap" in err()           # norms inside sol
        assert res(3, rhs, ld, sol, ld, rhs, ld) == 0                                               # r == rhs, same ld: allowed
        assert res(3, rhs, n - 1, sol, ld, out, ld) == -4 and "leading dimension" in err()
        assert res(0, rhs, ld, sol, ld, out, ld) == -4 and "nrhs" in err()
        ref_ = lambda nrhs, b, x, steps, nm=None: L.iem_kkt_solve_refined_diag(*common, nrhs, _p(b), ld, _p(x), ld, steps, _p(nm))
        assert ref_(3, rhs, out, 1) == -4 and "factorisation" in err()                              # not factorised yet
        assemble_diag(S, S.dd)
        factor(S)
        assert ref_(3, rhs, rhs, 1) == -4 and "overlap" in err()                                    # in place is refused here
        assert ref_(2, rhs, rhs[1:], 1) == -4 and "overlap" in err()
        assert ref_(3, rhs, out, 1, out[1, :6]) == -4 and "overlap" in err()
        assert ref_(3, rhs, out, -1) == -4 and "steps" in err()
        assert ref_(0, rhs, out, 1) == -4 and "nrhs" in err()
        assert ref_(3, rhs, out, 1) == 0
    # a sharded handle holds one rank's window: no object on it (and iem_kktprod, which the residuals go through, refuses it too)
    sm = ExaModel.sharded(dref.host_system("quadrotor_100")["blob"], 1, 0, 2, device=0)
    try:
        with pytest.raises(iemlib.IemError, match="sharded"):
            KKTObject(sm)
    finally:
        sm.close()


def test_kkt_object(built):
    """kkt_chain.KKTObject on quadrotor_100: solve((n, 3), refine = 1) bitwise the raw call, whatever the strides; residual and the
    unrefined solves likewise; sensitivity.parameter_steps accepts it as it accepts ChainKKT, and the two agree within ten times the
    solvers' own error against scipy's sparse LU on the same right-hand sides, measured in the run (the bound of
    tests/test_gpu_parameter_jacobian.py, floor 1e-15)."""
    import torch
    from scipy.sparse.linalg import splu
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.kkt import KKTSystem
    from infiniteexamodels.jl_amd.kkt_chain import ChainKKT, KKTObject
    from infiniteexamodels.jl_amd.sensitivity import parameter_steps
    with system("quadrotor_100") as S:
        n, gm = S.n, S.gm
        with KKTObject(gm) as obj:
            assert obj.info["n"] == n and obj.info["hubs"] == 0 and obj.set_border(1) is obj
            obj.assemble(S.hv, S.jv, S.sd, DW, DC, dcon=S.dd)
            inertia = obj.factor()
            assert inertia == (n - S.h["neg"], S.h["neg"], 0)
            with pytest.raises(ValueError, match="at="):
                obj.solve(S.B[0], refine=1)
            obj.assemble(S.hv, S.jv, S.sd, DW, DC, dcon=S.dd, at=(S.xd, S.yd, 1.0))
            assert obj.factor() == inertia
            assemble_diag(S, S.dd)      # the raw object of system(), the same matrix
            factor(S)
            rhs = padded(S.B[:3])
            cols = rhs[:, :n].t()       # (n, 3), columns ld apart
            assert not cols.is_contiguous()
            X = obj.solve(cols, refine=1)
            raw, _ = refined_diag(S, S.dd, rhs, 1, norms=False)
            assert X.shape == (n, 3) and torch.equal(_bits(X.t()), _bits(raw[:, :n]))
            assert torch.equal(_bits(obj.solve(S.B[0], refine=1)), _bits(raw[0, :n]))
            assert torch.equal(_bits(obj.solve(S.B[1])), _bits(solve(S, S.B[1]))) and torch.equal(_bits(obj.solve(cols).t()), _bits(solve_many(S, rhs)[:, :n]))
            assert torch.equal(_bits(obj.residual(cols, X).t()), _bits(residual_diag(S, S.dd, rhs, padded(X.t().contiguous()), norms=False)[0][:, :n]))
            # parameter sensitivities through it
            npar = S.h["om"].npar
            D = torch.tensor(np.random.default_rng(4).standard_normal((npar, 3)), device="cuda")
            kk = KKTSystem(gm)
            try:
                kk.assemble(S.hv, S.jv, S.sd, DW, S.dd + DC)
                ck = ChainKKT(kk).load().factor()
                got = torch.cat(parameter_steps(gm, obj, S.xd, S.yd, D)).cpu().numpy()
                want = torch.cat(parameter_steps(gm, ck, S.xd, S.yd, D)).cpu().numpy()
                # the solvers' own error: both against scipy on the right-hand sides parameter_steps builds
                buf = torch.empty(3, n, dtype=torch.float64, device="cuda")
                for j in range(3):
                    gm.hpprod(S.xd, S.yd, D[:, j].contiguous(), out=buf[j, :S.nvar])
                    gm.jpprod(S.xd, D[:, j].contiguous(), out=buf[j, S.nvar:])
                buf.neg_()
                exact = splu(S.h["K"].tocsc()).solve(buf.t().cpu().numpy())
                rel = lambda a, b: max(float(np.abs(a[:, j] - b[:, j]).max() / max(1.0, np.abs(b[:, j]).max())) for j in range(3))
                own = max(rel(obj.solve(buf.t()).cpu().numpy(), exact), rel(ck.solve(buf.t()).cpu().numpy(), exact))
                bound = 10.0 * max(own, 1e-15)
                print(f"quadrotor_100: the solvers' own error {own:.3e}, KKTObject against ChainKKT {rel(got, want):.3e} (bound {bound:.3e})")
                assert got.shape == (n, 3) and np.abs(want).max() > 0 and rel(got, want) <= bound
            finally:
                kk.close()
        obj.close()      # (a second close is a no-op)
        with pytest.raises(iemlib.IemError, match="closed"):
            obj.factor()
