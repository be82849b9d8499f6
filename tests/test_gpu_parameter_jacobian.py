"""sensitivity.parameter_jacobian on the MI355X through a factorised KKT system at a regularised point: column for column
what parameter_steps gives for the unit directions, without a single per-column product.

Two systems: the quadrotor at 300 supports (not a power of two) through a real ChainKKT, and shifted_pf(300) through
kkt.KKTSystem's sparse LU on the device — shifted_pf is a hand-built core without an infinite-parameter slab table, and the
chain analysis refuses such a model ("nothing to chain along"), so only the quadrotor takes the multi-column
ChainKKT.solve path.  The set-up is that of tests/test_gpu_adjoint_sensitivity.py (Σ from seed 3, δ_w = 1e-2, δ_c = 1e-6).

The two paths hand the solver right-hand sides that differ by the summation order of duplicate COO entries only, so the
bound is TEN TIMES THE SOLVER'S OWN ERROR at this size — code this feature does not change: for the right-hand side
``parameter_steps`` builds for the seven unit directions, max |solver − scipy's sparse LU of host_kkt| / max(1, |scipy|∞) per
column, the worst column (``solver_error``).  The test measures it in the run itself and takes ten times the larger of that
and a floor of 1e-15 (a few roundings of a unit-sized entry), so that a run in which both solvers happen to agree to the last
bit still leaves room for the rounding of the two right-hand sides.  No figure from an MI355X is recorded here yet: every
run prints the measured error, the bound and the gap of the two paths per column."""
import numpy as np
import pytest

import cases_param as CP
from pyoracle import OracleModel

pytestmark = pytest.mark.gpu
SOLVER_MEASURED = {"quadrotor_300": 1e-15, "shifted_pf_300": 1e-15}      # the floor of the bound; see above
_sys = {}


def system(name):
    if name not in _sys:
        import torch
        from infiniteexamodels.jl_amd import transcribe, workloads
        from infiniteexamodels.jl_amd.kkt import KKTSystem
        from infiniteexamodels.jl_amd.kkt_chain import ChainKKT
        from infiniteexamodels.jl_amd.model import ExaModel
        core = transcribe.exa_core(workloads.quadrotor(300)) if name == "quadrotor_300" else CP.shifted_pf(300)
        blob = core.to_blob()
        om = OracleModel(blob)
        gm = ExaModel(core, device=0, blob=blob)
        kkt = KKTSystem(gm)
        x = om.x0 + 0.1 * np.random.default_rng(5).standard_normal(om.nvar)
        y = np.random.default_rng(6).standard_normal(om.ncon)
        sigma = 0.5 + np.random.default_rng(3).random(om.nvar)
        xd, yd = torch.tensor(x, device="cuda"), torch.tensor(y, device="cuda")
        kkt.assemble(gm.hess_coord(xd, yd, obj_weight=1.0), gm.jac_coord(xd), torch.tensor(sigma, device="cuda"), 1e-2, 1e-6)
        if name == "quadrotor_300":
            solver = ChainKKT(kkt)
            solver.load().factor()
            S = 300
            cols = [0, S - 1, S, 2 * S - 1, 2 * S, 3 * S - 1, S]          # first and last entry of each of the three parameter functions, one repeated
        else:
            solver = kkt.analyse().factor()
            n = 300
            cols = [n, 0, n - 1, 1, 137, n, n - 2]                        # the finite parameter k (twice), first and last entry of pf, inner entries
        _sys[name] = dict(core=core, om=om, gm=gm, kkt=kkt, solver=solver, x=x, y=y, sigma=sigma, xd=xd, yd=yd, cols=cols)
    return _sys[name]


@pytest.fixture(scope="module")
def systems(built):
    yield system
    for s in _sys.values():
        s["kkt"].close(); s["gm"].close()
    _sys.clear()


def unit_directions(s):
    import torch
    D = torch.zeros(s["om"].npar, len(s["cols"]), dtype=torch.float64, device="cuda")
    for k, c in enumerate(s["cols"]):
        D[c, k] = 1.0
    return D


def solver_error(s):
    """What SOLVER_MEASURED records: the solver against scipy's sparse LU on the right-hand side parameter_steps builds —
    nothing of the feature is in it."""
    import torch
    from scipy.sparse.linalg import splu
    from test_kkt import host_kkt
    gm, n, mc = s["gm"], s["om"].nvar, s["om"].ncon
    D = unit_directions(s)
    rhs = torch.empty(D.shape[1], n + mc, dtype=torch.float64, device="cuda")
    for j in range(D.shape[1]):
        gm.hpprod(s["xd"], s["yd"], D[:, j].contiguous(), out=rhs[j, :n])
        gm.jpprod(s["xd"], D[:, j].contiguous(), out=rhs[j, n:])
    rhs.neg_()
    got = s["solver"].solve(rhs.t()).cpu().numpy()
    want = splu(host_kkt(s["om"], s["x"], s["y"], s["sigma"], 1e-2, 1e-6).tocsc()).solve(rhs.t().cpu().numpy())
    return max(float(np.abs(got[:, j] - want[:, j]).max() / max(1.0, np.abs(want[:, j]).max())) for j in range(D.shape[1]))


@pytest.mark.parametrize("name", ["quadrotor_300", "shifted_pf_300"])
def test_jacobian_equals_the_unit_steps(name, systems):
    from infiniteexamodels.jl_amd.sensitivity import parameter_jacobian, parameter_steps
    s = systems(name)
    gm = s["gm"]
    measured = solver_error(s)
    bound = 10.0 * max(measured, SOLVER_MEASURED[name])
    print(f"{name}: the solver's own error {measured:.3e} (floor {SOLVER_MEASURED[name]:.1e})")
    sX, sY = parameter_steps(gm, s["solver"], s["xd"], s["yd"], unit_directions(s))
    counts = {"jpprod": 0, "hpprod": 0}
    real = {k: getattr(gm, k) for k in counts}

    def counting(k):
        def f(*a, **kw):
            counts[k] += 1
            return real[k](*a, **kw)
        return f
    for k in counts:
        setattr(gm, k, counting(k))
    try:
        dX, dY = parameter_jacobian(gm, s["solver"], s["xd"], s["yd"], s["cols"])
    finally:
        for k in counts:
            delattr(gm, k)
    assert counts == {"jpprod": 0, "hpprod": 0}      # no per-column product
    assert dX.shape == sX.shape and dY.shape == sY.shape
    got = np.concatenate([dX.cpu().numpy(), dY.cpu().numpy()])
    want = np.concatenate([sX.cpu().numpy(), sY.cpu().numpy()])
    errs = [float(np.abs(got[:, j] - want[:, j]).max() / max(1.0, np.abs(want[:, j]).max())) for j in range(len(s["cols"]))]
    print(f"{name}: parameter_jacobian against parameter_steps, per column:", " ".join(f"{e:.3e}" for e in errs), f"(bound {bound:.3e})")
    assert all(np.abs(want[:, j]).max() > 0 for j in range(len(s["cols"])))
    assert max(errs) <= bound
    rep = [k for k, c in enumerate(s["cols"]) if s["cols"].count(c) > 1]
    np.testing.assert_array_equal(got[:, rep[0]], got[:, rep[1]])      # the repeated index: the same column twice
    again = parameter_jacobian(gm, s["solver"], s["xd"], s["yd"], s["cols"])
    assert np.array_equal(again[0].cpu().numpy(), dX.cpu().numpy())     # one plan per (model, cols), the same bits
