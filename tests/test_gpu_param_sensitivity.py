"""Parameter sensitivities on the MI355X: the C-ABI entries iem_jpprod / iem_jptprod / iem_hpprod (through
model.ExaModel) against witness A (torch float64 autograd on the CPU, tests/param_witness.py) to the 1e-10 relative of
the parity suite, bit-reproducibility over repeated calls, θ updates, the sharded refusal — and sensitivity.parameter_step
through a real chain KKT solve."""
import ctypes as C

import numpy as np
import pytest

import cases
import cases_param as CP
from param_witness import WitnessA
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
def test_cabi_matches_autograd_and_is_reproducible(name, grid_mode):
    import torch
    from infiniteexamodels.jl_amd.model import ExaModel
    core = CP.build_core(name)
    blob = core.to_blob()
    om = OracleModel(blob)
    gm = ExaModel(core, device=0, blob=blob)
    A = WitnessA(core)
    try:
        for seed in (0, 1):
            x, y = CP.eval_point(name, om, seed)
            w = np.random.default_rng(3 + seed).standard_normal(om.npar)
            sigma = 0.7 + 0.6 * seed
            xd, yd, wd = (torch.tensor(a, device="cuda") for a in (x, y, w))
            jp = gm.jpprod(xd, wd, out=_poisoned(om.ncon))
            jpt = gm.jptprod(xd, yd, obj_weight=sigma, out=_poisoned(om.npar))
            hp = gm.hpprod(xd, yd, wd, obj_weight=sigma, out=_poisoned(om.nvar))
            errs = {"jpprod": rel(jp.cpu().numpy(), A.jpprod(x, w)), "jptprod": rel(jpt.cpu().numpy(), A.jptprod(x, y, sigma)),
                    "hpprod": rel(hp.cpu().numpy(), A.hpprod(x, y, w, sigma))}
            print(name, seed, errs)
            assert max(errs.values()) <= TOL, errs
            for _ in range(10):      # identical bits, call after call
                assert torch.equal(gm.jpprod(xd, wd, out=_poisoned(om.ncon)).view(torch.int64), jp.view(torch.int64))
                assert torch.equal(gm.jptprod(xd, yd, obj_weight=sigma, out=_poisoned(om.npar)).view(torch.int64), jpt.view(torch.int64))
                assert torch.equal(gm.hpprod(xd, yd, wd, obj_weight=sigma, out=_poisoned(om.nvar)).view(torch.int64), hp.view(torch.int64))
        # the kernels ran from the offline build, and report their traffic
        ks = gm.param_kernels()
        assert any(k["name"].startswith("iem_jpprod") and k["alg_bytes_written"] >= 8 * om.ncon for k in ks)
        assert not any(k["jit"] for k in gm.kernels()), "the parameter kinds were compiled at run time: build() must precompile them"
        # a call after iem_set_parameter sees the new θ
        th2 = np.asarray(core.theta) * 1.1 + 0.05
        gm.set_parameter(0, th2)
        A2 = WitnessA(core, th2)
        x, y = CP.eval_point(name, om, 0)
        w = np.random.default_rng(3).standard_normal(om.npar)
        xd, yd, wd = (torch.tensor(a, device="cuda") for a in (x, y, w))
        assert rel(gm.jpprod(xd, wd).cpu().numpy(), A2.jpprod(x, w)) <= TOL
        assert rel(gm.jptprod(xd, yd, obj_weight=0.7).cpu().numpy(), A2.jptprod(x, y, 0.7)) <= TOL
        assert rel(gm.hpprod(xd, yd, wd, obj_weight=0.7).cpu().numpy(), A2.hpprod(x, y, w, 0.7)) <= TOL
        # ... and the check can tell: by the witness alone, the new θ moves at least one of the three products
        # (rosenbrock's mixed derivative is constant in θ, its ∇θL is not)
        if name in ("rosenbrock", "shifted_pf", "pfun"):
            assert max(rel(A2.jpprod(x, w), A.jpprod(x, w)), rel(A2.jptprod(x, y, 0.7), A.jptprod(x, y, 0.7)),
                       rel(A2.hpprod(x, y, w, 0.7), A.hpprod(x, y, w, 0.7))) > 1e-6
    finally:
        gm.close()


@pytest.mark.parametrize("name", CP.NO_PARAM)
def test_no_parameters_on_gpu(name, built):
    import torch
    from infiniteexamodels.jl_amd.model import ExaModel
    core = CP.build_core(name)
    gm = ExaModel(core, device=0)
    try:
        assert gm.meta.npar == 0
        x = torch.tensor(gm.meta.x0, device="cuda")
        y = torch.ones(gm.meta.ncon, dtype=torch.float64, device="cuda")
        w = torch.empty(0, dtype=torch.float64, device="cuda")
        assert torch.equal(gm.jpprod(x, w, out=_poisoned(gm.meta.ncon)), torch.zeros_like(y))
        assert torch.equal(gm.hpprod(x, y, w, out=_poisoned(gm.meta.nvar)), torch.zeros_like(x))
        assert gm.jptprod(x, y).numel() == 0
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
        for rc in (L.iem_jpprod(sm._h, x.data_ptr(), w.data_ptr(), y.data_ptr()),
                   L.iem_jptprod(sm._h, x.data_ptr(), y.data_ptr(), 1.0, w.data_ptr()),
                   L.iem_hpprod(sm._h, x.data_ptr(), y.data_ptr(), 1.0, w.data_ptr(), x.data_ptr())):
            assert rc == -4      # IEM_E_ARG
            msg = L.iem_last_error().decode()
            assert "sharded" in msg and "all-reduce" in msg and "out of scope" in msg
        with pytest.raises(iemlib.IemError, match="sharded"):
            sm.jpprod(x, w)
    finally:
        sm.close()


# The chain solver against scipy on THIS system (quadrotor, 1 000 supports, sigma / delta_w = 1e-2 / delta_c = 1e-6 as in
# tests/test_kkt_chain.py::test_chain_kkt_on_gpu[quadrotor_1000], random right-hand side, refine = 1), measured on an
# MI355X (the KKT classes are untouched by this feature): max |sol − scipy| / max(1, |scipy|∞) = 8.27e-14 (seed 5) and 3.35e-13
# (seed 9), residuals 3.0e-12 / 2.8e-12 at max |scipy| 1.2e4 / 8.8e3.  CHAIN_MEASURED is the worse of the two.
CHAIN_MEASURED = 3.346e-13
CHAIN_BOUND = 10.0 * CHAIN_MEASURED


def test_parameter_step_through_the_chain_solver(built):
    """parameter_step through a real ChainKKT on the quadrotor at 1 000 supports against the dense answer: K from the
    oracle, the right-hand side from witness A, scipy's sparse LU.  Bound: ten times what the chain solve itself reaches
    against scipy at this size (CHAIN_MEASURED = 3.346e-13 above, from the existing solve — not from the code under test;
    CHAIN_BOUND = 3.346e-12)."""
    import torch
    from scipy.sparse.linalg import spsolve
    from infiniteexamodels.jl_amd.kkt import KKTSystem
    from infiniteexamodels.jl_amd.kkt_chain import ChainKKT
    from infiniteexamodels.jl_amd.model import ExaModel
    from infiniteexamodels.jl_amd.sensitivity import parameter_step
    from test_kkt import host_kkt
    core = cases.build_core("quadrotor_1000")
    blob = core.to_blob()
    om = OracleModel(blob)
    gm = ExaModel(core, device=0, blob=blob)
    kkt = KKTSystem(gm)
    ck = ChainKKT(kkt)
    try:
        x, y = cases.eval_point_for("quadrotor_1000", om, 5)
        rng = np.random.default_rng(3)
        sigma = 0.5 + rng.random(om.nvar)
        dth = 0.1 * rng.standard_normal(om.npar)
        xd, yd = torch.tensor(x, device="cuda"), torch.tensor(y, device="cuda")
        kkt.assemble(gm.hess_coord(xd, yd, obj_weight=1.0), gm.jac_coord(xd), torch.tensor(sigma, device="cuda"), 1e-2, 1e-6)
        ck.load().factor()
        dx, dy = parameter_step(gm, ck, xd, yd, torch.tensor(dth, device="cuda"))
        A = WitnessA(core)
        rhs = -np.concatenate([A.hpprod(x, y, dth, 1.0), A.jpprod(x, dth)])
        want = spsolve(host_kkt(om, x, y, sigma, 1e-2, 1e-6).tocsc(), rhs)
        got = np.concatenate([dx.cpu().numpy(), dy.cpu().numpy()])
        err = np.abs(got - want).max() / max(1.0, np.abs(want).max())
        print(f"parameter_step through ChainKKT: {err:.3e} (bound {CHAIN_BOUND:.3e}), max |step| {np.abs(want).max():.3e}")
        assert np.abs(want).max() > 0 and err <= CHAIN_BOUND
    finally:
        kkt.close(); gm.close()
