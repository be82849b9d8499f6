"""The adjoint parameter kind on the MI355X: iem_hptprod through model.ExaModel against torch float64 autograd on the CPU
(tests/adjoint_witness.py) to the 1e-10 relative of the parity suite, bit-reproducibility over repeated calls, θ updates,
the sharded refusal — and sensitivity.parameter_gradient(s) through a real chain KKT solve."""
import numpy as np
import pytest

import cases
import cases_param as CP
from adjoint_witness import WitnessAdjoint
from pyoracle import OracleModel

pytestmark = pytest.mark.gpu
TOL = 1e-10


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape
    if a.size == 0:
        return 0.0
    assert np.isfinite(a).all(), "an output entry was never written"
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


def _poisoned(n):
    import torch
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


@pytest.mark.parametrize("name", CP.NAMES)
def test_hptprod_matches_autograd_and_is_reproducible(name, grid_mode):
    import torch
    from infiniteexamodels.jl_amd.model import ExaModel
    core = CP.build_core(name)
    blob = core.to_blob()
    om = OracleModel(blob)
    gm = ExaModel(core, device=0, blob=blob)
    A = WitnessAdjoint(core)
    try:
        for seed in (0, 1):
            x, y = CP.eval_point(name, om, seed)
            u = np.random.default_rng(11 + seed).standard_normal(om.nvar)
            sigma = 0.7 + 0.6 * seed
            xd, yd, ud = (torch.tensor(a, device="cuda") for a in (x, y, u))
            got = gm.hptprod(xd, yd, ud, obj_weight=sigma, out=_poisoned(om.npar))
            err = rel(got.cpu().numpy(), A.hptprod(x, y, u, sigma))
            print(name, seed, grid_mode, err)
            assert err <= TOL
            for _ in range(10):      # identical bits, call after call
                assert torch.equal(gm.hptprod(xd, yd, ud, obj_weight=sigma, out=_poisoned(om.npar)).view(torch.int64), got.view(torch.int64))
        # the kernels ran from the offline build, and are listed behind the other parameter kinds
        names = [k["name"] for k in gm.param_kernels()]
        first = min(i for i, n in enumerate(names) if n.startswith("iem_hptprod"))
        assert all(n.startswith("iem_hptprod") for n in names[first:]) and not any(n.startswith("iem_hptprod") for n in names[:first])
        assert any(n.startswith("iem_jpprod") for n in names[:first])
        assert not any(k["jit"] for k in gm.kernels()), "hptprod was compiled at run time: build() must precompile it"
        # a call after iem_set_parameter sees the new θ
        th2 = np.asarray(core.theta) * 1.1 + 0.05
        gm.set_parameter(0, th2)
        A2 = WitnessAdjoint(core, th2)
        x, y = CP.eval_point(name, om, 0)
        u = np.random.default_rng(11).standard_normal(om.nvar)
        xd, yd, ud = (torch.tensor(a, device="cuda") for a in (x, y, u))
        assert rel(gm.hptprod(xd, yd, ud, obj_weight=0.7).cpu().numpy(), A2.hptprod(x, y, u, 0.7)) <= TOL
        if name == "shifted_pf":      # ... and the check can tell, by the witness alone (its mixed derivative depends on θ)
            assert rel(A2.hptprod(x, y, u, 0.7), A.hptprod(x, y, u, 0.7)) > 1e-6
    finally:
        gm.close()


@pytest.mark.parametrize("name", CP.NO_PARAM)
def test_no_parameters_on_gpu(name, built):
    import torch
    from infiniteexamodels.jl_amd.model import ExaModel
    gm = ExaModel(CP.build_core(name), device=0)
    try:
        assert gm.meta.npar == 0
        x = torch.tensor(gm.meta.x0, device="cuda")
        y = torch.ones(gm.meta.ncon, dtype=torch.float64, device="cuda")
        assert gm.hptprod(x, y, torch.ones_like(x)).numel() == 0
        assert not any(k["name"].startswith("iem_hptprod") for k in gm.param_kernels())
    finally:
        gm.close()


def test_sharded_handle_refuses(built):
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd import transcribe, workloads
    from infiniteexamodels.jl_amd.model import ExaModel
    blob = transcribe.exa_core(workloads.quadrotor(4000)).to_blob()
    sm = ExaModel.sharded(blob, 1, 1, 2, device=0)
    try:
        x = torch.zeros(sm.meta.nvar, dtype=torch.float64, device="cuda")
        y = torch.zeros(sm.meta.ncon, dtype=torch.float64, device="cuda")
        w = torch.zeros(sm.meta.npar, dtype=torch.float64, device="cuda")
        L = iemlib.lib()
        assert L.iem_hptprod(sm._h, x.data_ptr(), y.data_ptr(), 1.0, x.data_ptr(), w.data_ptr()) == -4      # IEM_E_ARG
        msg = L.iem_last_error().decode()
        assert "iem_hptprod" in msg and "sharded" in msg and "all-reduce" in msg and "out of scope" in msg
        with pytest.raises(iemlib.IemError, match="sharded"):
            sm.hptprod(x, y, x)
    finally:
        sm.close()


# The bound of the two chain-solver tests below is the EXISTING ChainKKT.solve's own error carried through an exact product —
# code this feature does not change: on the system of test_gpu_param_sensitivity.py::test_parameter_step_through_the_chain_solver
# (quadrotor, 1 000 supports, point seed 5, Σ from seed 3, δ_w = 1e-2, δ_c = 1e-6) and the right-hand side g = column 0 of
# _rhs_columns() below, λ_chain = ChainKKT.solve(g) and λ_scipy = scipy's sparse LU on host_kkt; the difference is pushed
# through witness A's Gᵀ on the CPU (linear in λ): max |Gᵀ(λ_chain − λ_scipy)| / max(1, |Gᵀλ_scipy|∞), measured on an MI355X:
#   column 0 (the g of the single gradient): 2.005e-13          columns 1 - 4: 2.608e-13, 2.952e-13, 1.493e-13, 1.768e-13
# at max |Gᵀλ_scipy| = 4.59 (3.4 - 4.2 for the other columns).  The bound of every column is ten times the value of column 0.
CHAIN_GT_MEASURED = 2.005e-13
CHAIN_GT_BOUND = 10.0 * CHAIN_GT_MEASURED
K_COLS = 5


def _rhs_columns(n, m):
    return np.random.default_rng(21).standard_normal((n + m, K_COLS))


_chain = {}


def chain_system():
    """The factorised chain KKT system, scipy's λ for every column of the right-hand sides and witness A's Gᵀλ — built
    once, shared by the two tests (and by whoever re-measures CHAIN_GT_MEASURED)."""
    if not _chain:
        import torch
        from scipy.sparse.linalg import splu
        from infiniteexamodels.jl_amd.kkt import KKTSystem
        from infiniteexamodels.jl_amd.kkt_chain import ChainKKT
        from infiniteexamodels.jl_amd.model import ExaModel
        from test_kkt import host_kkt
        core = cases.build_core("quadrotor_1000")
        blob = core.to_blob()
        om = OracleModel(blob)
        gm = ExaModel(core, device=0, blob=blob)
        kkt = KKTSystem(gm)
        ck = ChainKKT(kkt)
        x, y = cases.eval_point_for("quadrotor_1000", om, 5)
        sigma = 0.5 + np.random.default_rng(3).random(om.nvar)
        xd, yd = torch.tensor(x, device="cuda"), torch.tensor(y, device="cuda")
        kkt.assemble(gm.hess_coord(xd, yd, obj_weight=1.0), gm.jac_coord(xd), torch.tensor(sigma, device="cuda"), 1e-2, 1e-6)
        ck.load().factor()
        G = _rhs_columns(om.nvar, om.ncon)
        lam = splu(host_kkt(om, x, y, sigma, 1e-2, 1e-6).tocsc()).solve(G)
        A = WitnessAdjoint(core)
        want = np.stack([-A.gt_lambda(x, y, lam[:, j], 1.0) for j in range(K_COLS)], axis=1)
        _chain.update(om=om, gm=gm, kkt=kkt, ck=ck, x=x, y=y, xd=xd, yd=yd, G=G, lam=lam, A=A, want=want)
    return _chain


def chain_solver_error_through_gt(j=0):
    """What CHAIN_GT_MEASURED records (column j): nothing of the feature is in it."""
    import torch
    s = chain_system()
    lam_chain = s["ck"].solve(torch.tensor(s["G"][:, j].copy(), device="cuda")).cpu().numpy()
    diff = s["A"].gt_lambda(s["x"], s["y"], lam_chain - s["lam"][:, j], 1.0)
    return float(np.abs(diff).max() / max(1.0, np.abs(s["want"][:, j]).max()))


@pytest.fixture(scope="module")
def chain(built):
    yield chain_system()
    if _chain:
        _chain["kkt"].close(); _chain["gm"].close()
        _chain.clear()


def test_parameter_gradient_through_the_chain_solver(chain):
    """parameter_gradient through a real ChainKKT on the quadrotor at 1 000 supports against the dense answer (λ from scipy's
    sparse LU, Gᵀλ from witness A); bound: ten times the solver's own error carried through Gᵀ (CHAIN_GT_MEASURED above)."""
    import torch
    from infiniteexamodels.jl_amd.sensitivity import parameter_gradient
    s, n = chain, chain["om"].nvar
    print(f"solver's own error through G': {chain_solver_error_through_gt(0):.3e} (recorded {CHAIN_GT_MEASURED})")
    g = s["G"][:, 0]
    got = parameter_gradient(s["gm"], s["ck"], s["xd"], s["yd"], torch.tensor(g[:n].copy(), device="cuda"), torch.tensor(g[n:].copy(), device="cuda"))
    want = s["want"][:, 0]
    err = rel(got.cpu().numpy(), want)
    print(f"parameter_gradient through ChainKKT: {err:.3e} (bound {CHAIN_GT_BOUND}), max |gradient| {np.abs(want).max():.3e}")
    assert np.abs(want).max() > 0
    assert err <= CHAIN_GT_BOUND


def test_parameter_gradients_through_the_chain_solver(chain):
    """K = 5 quantities: one ChainKKT.solve with a 2-D right-hand side, every column to the bound of the single gradient."""
    import torch
    from infiniteexamodels.jl_amd.sensitivity import parameter_gradients
    s = chain
    calls = []
    solve = s["ck"].solve

    class Counting:
        def solve(self, rhs):
            calls.append(tuple(rhs.shape))
            return solve(rhs)
    got = parameter_gradients(s["gm"], Counting(), s["xd"], s["yd"], torch.tensor(s["G"], device="cuda")).cpu().numpy()
    assert calls == [(s["G"].shape[0], K_COLS)] and got.shape == s["want"].shape
    errs = [rel(got[:, j], s["want"][:, j]) for j in range(K_COLS)]
    print("parameter_gradients through ChainKKT:", " ".join(f"{e:.3e}" for e in errs), f"(bound {CHAIN_GT_BOUND})")
    assert all(np.abs(s["want"][:, j]).max() > 0 for j in range(K_COLS))
    assert max(errs) <= CHAIN_GT_BOUND
