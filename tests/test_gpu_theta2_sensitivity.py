"""The θθ parameter kind on the MI355X: iem_hppprod through model.ExaModel against torch float64 autograd on the CPU
(tests/theta2_witness.py) to the 1e-10 relative of the parity suite, bit-reproducibility over repeated calls, θ updates,
the sharded refusal, a graph capture — and sensitivity.value_hessian_product(s) through a real chain KKT solve."""
import numpy as np
import pytest

import cases
import cases_param as CP
from pyoracle import OracleModel
from test_gpu_adjoint_sensitivity import chain_system
from theta2_witness import WitnessTheta2

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
def test_hppprod_matches_autograd_and_is_reproducible(name, grid_mode):
    import torch
    from infiniteexamodels.jl_amd.model import ExaModel
    core = CP.build_core(name)
    blob = core.to_blob()
    om = OracleModel(blob)
    gm = ExaModel(core, device=0, blob=blob)
    A = WitnessTheta2(core)
    try:
        for seed in (0, 1):
            x, y = CP.eval_point(name, om, seed)
            w = np.random.default_rng(3 + seed).standard_normal(om.npar)
            sigma = 0.7 + 0.6 * seed
            xd, yd, wd = (torch.tensor(a, device="cuda") for a in (x, y, w))
            got = gm.hppprod(xd, yd, wd, obj_weight=sigma, out=_poisoned(om.npar))
            want = A.hppprod(x, y, w, sigma)
            err = rel(got.cpu().numpy(), want)
            print(name, seed, grid_mode, err, "max |want|", np.abs(want).max())
            assert (np.abs(want).max() > 0) == (name != "quadrotor_1")
            assert err <= TOL
            for _ in range(10):      # identical bits, call after call
                assert torch.equal(gm.hppprod(xd, yd, wd, obj_weight=sigma, out=_poisoned(om.npar)).view(torch.int64), got.view(torch.int64))
        # the kernels ran from the offline build, and are a program of their own behind the other parameter kinds
        mine = gm.hppprod_kernels()
        assert mine and all(k["name"].startswith("iem_hppprod") for k in mine)
        assert not any(k["name"].startswith("iem_hppprod") for k in gm.param_kernels())
        assert not any(k["jit"] for k in gm.kernels() + mine), "hppprod was compiled at run time: build() must precompile it"
        # a call after iem_set_parameter sees the new θ
        th2 = np.asarray(core.theta) * 1.1 + 0.05
        gm.set_parameter(0, th2)
        A2 = WitnessTheta2(core, th2)
        x, y = CP.eval_point(name, om, 0)
        w = np.random.default_rng(3).standard_normal(om.npar)
        xd, yd, wd = (torch.tensor(a, device="cuda") for a in (x, y, w))
        assert rel(gm.hppprod(xd, yd, wd, obj_weight=0.7).cpu().numpy(), A2.hppprod(x, y, w, 0.7)) <= TOL
        if name == "shifted_pf":      # ... and the check can tell, by the witness alone (its θθ block depends on θ)
            assert rel(A2.hppprod(x, y, w, 0.7), A.hppprod(x, y, w, 0.7)) > 1e-6
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
        assert gm.hppprod(x, y, torch.zeros(0, dtype=torch.float64, device="cuda")).numel() == 0
        assert gm.hppprod_prepare() == 0 and gm.hppprod_kernels() == []
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
        assert L.iem_hppprod(sm._h, x.data_ptr(), y.data_ptr(), 1.0, w.data_ptr(), w.data_ptr()) == -4      # IEM_E_ARG
        msg = L.iem_last_error().decode()
        assert "iem_hppprod" in msg and "sharded" in msg and "all-reduce" in msg and "out of scope" in msg
        with pytest.raises(iemlib.IemError, match="sharded"):
            sm.hppprod(x, y, w)
        with pytest.raises(iemlib.IemError, match="sharded"):
            sm.hppprod_prepare()
    finally:
        sm.close()


def test_later_calls_are_capturable(built):
    """hppprod_prepare() does the synchronous set-up; a call after it is recorded into a (single-branch) graph and replays
    to the bits of the eager call."""
    import torch
    from infiniteexamodels.jl_amd.model import ExaModel
    core = CP.build_core("shifted_pf")
    blob = core.to_blob()
    om = OracleModel(blob)
    gm = ExaModel(core, device=0, blob=blob)
    try:
        x, y = CP.eval_point("shifted_pf", om, 0)
        w = np.random.default_rng(3).standard_normal(om.npar)
        xd, yd, wd = (torch.tensor(a, device="cuda") for a in (x, y, w))
        assert gm.hppprod_prepare() > 0
        eager = gm.hppprod(xd, yd, wd, obj_weight=0.7, out=_poisoned(om.npar)).clone()
        assert rel(eager.cpu().numpy(), WitnessTheta2(core).hppprod(x, y, w, 0.7)) <= TOL
        out = _poisoned(om.npar)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            gm.hppprod(xd, yd, wd, obj_weight=0.7, out=out)
        for _ in range(2):
            out.fill_(float("nan"))
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out.view(torch.int64), eager.view(torch.int64))
    finally:
        gm.close()


# The bound of the two chain-solver tests below is the EXISTING ChainKKT.solve's own error carried through an exact product —
# code this feature does not change: on the system of test_gpu_adjoint_sensitivity.py::chain_system (quadrotor, 1 000
# supports, point seed 5, Σ from seed 3, δ_w = 1e-2, δ_c = 1e-6) and the right-hand sides −G·δθ (δθ = the K_COLS columns of
# _directions() below, G·δθ from witness A's hpprod / jpprod), sol_chain = ChainKKT.solve(rhs) and sol_scipy = scipy's sparse LU
# on host_kkt; the difference is pushed through witness A's Gᵀ on the CPU (linear in sol):
# max |Gᵀ(sol_chain − sol_scipy)| / max(1, |want|∞), measured on an MI355X:
#   column 0 (the δθ of the single product): 1.709e-16          columns 1 - 2: 2.206e-16, 1.727e-16
# at max |want| = 0.462 (0.444, 0.607 for the other columns: below 1, so the figure is an absolute error) — the rounding level of
# float64, because the step a change of the reference trajectory causes is small (max |step| 0.2) and G is a short stencil.
# The bound of every column is ten times the value of column 0.
CHAIN_VH_MEASURED = 1.709e-16
CHAIN_VH_BOUND = 10.0 * CHAIN_VH_MEASURED
K_COLS = 3

_vh = {}


def _directions(npar):
    return np.random.default_rng(31).standard_normal((npar, K_COLS))


def value_hessian_system():
    """chain_system() plus, for every column of _directions(): the right-hand side −G·δθ, scipy's solution of it and the
    dense answer L_θθ·δθ + Gᵀ·sol, all from witness A — built once, shared by the two tests (and by whoever re-measures
    CHAIN_VH_MEASURED)."""
    if not _vh:
        from scipy.sparse.linalg import splu
        from test_kkt import host_kkt
        s = chain_system()
        om, x, y = s["om"], s["x"], s["y"]
        A = WitnessTheta2(cases.build_core("quadrotor_1000"))
        D = _directions(om.npar)
        rhs = -np.stack([np.concatenate([A.hpprod(x, y, D[:, j], 1.0), A.jpprod(x, D[:, j])]) for j in range(K_COLS)], axis=1)
        sigma = 0.5 + np.random.default_rng(3).random(om.nvar)      # (the Σ chain_system assembled with)
        sol = splu(host_kkt(om, x, y, sigma, 1e-2, 1e-6).tocsc()).solve(rhs)
        want = np.stack([A.hppprod(x, y, D[:, j], 1.0) + A.gt_lambda(x, y, sol[:, j], 1.0) for j in range(K_COLS)], axis=1)
        _vh.update(s=s, A=A, D=D, rhs=rhs, sol=sol, want=want)
    return _vh


def chain_solver_error_through_gt(j=0):
    """What CHAIN_VH_MEASURED records (column j): nothing of the feature is in it."""
    import torch
    v = value_hessian_system()
    s = v["s"]
    sol_chain = s["ck"].solve(torch.tensor(v["rhs"][:, j].copy(), device="cuda")).cpu().numpy()
    diff = v["A"].gt_lambda(s["x"], s["y"], sol_chain - v["sol"][:, j], 1.0)
    return float(np.abs(diff).max() / max(1.0, np.abs(v["want"][:, j]).max()))


@pytest.fixture(scope="module")
def vh(built):
    from test_gpu_adjoint_sensitivity import _chain
    yield value_hessian_system()
    if _chain:
        _chain["kkt"].close(); _chain["gm"].close()
        _chain.clear()
    _vh.clear()


def test_value_hessian_product_through_the_chain_solver(vh):
    """value_hessian_product through a real ChainKKT on the quadrotor at 1 000 supports against the dense answer (the step
    from scipy's sparse LU, every product from witness A); bound: ten times the solver's own error carried through Gᵀ
    (CHAIN_VH_MEASURED above)."""
    import torch
    from infiniteexamodels.jl_amd.sensitivity import value_hessian_product
    s = vh["s"]
    print("solver's own error through G':", " ".join(f"{chain_solver_error_through_gt(j):.3e}" for j in range(K_COLS)),
          f"(recorded {CHAIN_VH_MEASURED}); max |want|", " ".join(f"{np.abs(vh['want'][:, j]).max():.3e}" for j in range(K_COLS)))
    got = value_hessian_product(s["gm"], s["ck"], s["xd"], s["yd"], torch.tensor(vh["D"][:, 0].copy(), device="cuda"))
    want = vh["want"][:, 0]
    err = rel(got.cpu().numpy(), want)
    print(f"value_hessian_product through ChainKKT: {err:.3e} (bound {CHAIN_VH_BOUND}), max |want| {np.abs(want).max():.3e}")
    assert np.abs(want).max() > 0
    assert err <= CHAIN_VH_BOUND


def test_value_hessian_products_through_the_chain_solver(vh):
    """K = 3 directions: one ChainKKT.solve with a 2-D right-hand side, every column to the bound of the single product."""
    import torch
    from infiniteexamodels.jl_amd.sensitivity import value_hessian_products
    s = vh["s"]
    calls = []
    solve = s["ck"].solve

    class Counting:
        def solve(self, rhs):
            calls.append(tuple(rhs.shape))
            return solve(rhs)
    got = value_hessian_products(s["gm"], Counting(), s["xd"], s["yd"], torch.tensor(vh["D"], device="cuda")).cpu().numpy()
    assert calls == [(vh["rhs"].shape[0], K_COLS)] and got.shape == vh["want"].shape
    errs = [rel(got[:, j], vh["want"][:, j]) for j in range(K_COLS)]
    print("value_hessian_products through ChainKKT:", " ".join(f"{e:.3e}" for e in errs), f"(bound {CHAIN_VH_BOUND})")
    assert all(np.abs(vh["want"][:, j]).max() > 0 for j in range(K_COLS))
    assert max(errs) <= CHAIN_VH_BOUND
