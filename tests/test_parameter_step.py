"""sensitivity.parameter_step and ExaTranscriptionBackend.parameter_direction on the CPU.

The step is pure linear algebra behind two matrix-free products: K is assembled densely from the ORACLE's jac_coord /
hess_coord, the right-hand side −[∇²ₓθL·δθ ; ∂c/∂θ·δθ] comes from witness A (torch autograd, tests/param_witness.py) and
scipy solves.  parameter_step gets the generated kernels (compiled for the host, tests/emu_param.py) behind the method
names of model.ExaModel and a stub `kkt` whose solve IS that scipy solve: the two answers agree to 1e-10 relative.

K = [H + δw·I, Jᵀ; J, −δc·I] with δw = δc = 1e-2: the parameter-function model has more (inequality) rows than
variables, so the unregularised matrix is singular; the regularised one is what a solver factorises, and its condition
number (≤ 1e6 here) times the 1e-16 of the right-hand sides stays five orders below the tolerance."""
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.linalg

import cases
from emu_param import EmulatedParamModel
from infiniteexamodels.jl_amd import transcribe, workloads
from infiniteexamodels.jl_amd.sensitivity import parameter_step
from param_witness import WitnessA
from pyoracle import OracleModel
from test_kkt import host_kkt

TOL = 1e-10


class HostParamModel:
    """The emulated kernels behind ExaModel's method names (torch CPU tensors)."""

    def __init__(self, core, blob):
        self.em = EmulatedParamModel(core, blob)
        self.meta = SimpleNamespace(nvar=self.em.nvar, ncon=self.em.ncon, npar=self.em.npar)

    def hpprod(self, x, y, w, obj_weight=1.0, out=None):
        import torch
        v = torch.from_numpy(self.em.hpprod(x.numpy(), y.numpy(), w.numpy(), obj_weight).copy())
        return v if out is None else out.copy_(v)

    def jpprod(self, x, w, out=None):
        import torch
        v = torch.from_numpy(self.em.jpprod(x.numpy(), w.numpy()).copy())
        return v if out is None else out.copy_(v)


class ScipyKKT:
    def __init__(self, K):
        self.lu = scipy.linalg.lu_factor(K)
        self.calls = 0

    def solve(self, rhs):
        import torch
        self.calls += 1
        return torch.from_numpy(scipy.linalg.lu_solve(self.lu, rhs.numpy()))


def _cores():
    return {"quadrotor_11": lambda: transcribe.exa_core(workloads.quadrotor(11)), "pfun": lambda: cases.build_core("pfun")}


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("name", ["quadrotor_11", "pfun"])
def test_parameter_step_matches_dense_solve(name, seed, built):
    import torch
    core = _cores()[name]()
    blob = core.to_blob()
    om = OracleModel(blob)
    assert om.npar > 0
    rng = np.random.default_rng(20 + seed)
    x = om.x0 + 0.1 * rng.standard_normal(om.nvar)
    y = rng.standard_normal(om.ncon)
    dth = 0.1 * rng.standard_normal(om.npar)
    sigma = 1.0 if seed == 0 else 0.6
    K = host_kkt(om, x, y, np.zeros(om.nvar), 1e-2, 1e-2, w=sigma).toarray()
    assert np.linalg.cond(K) <= 1e6
    A = WitnessA(core)
    rhs = -np.concatenate([A.hpprod(x, y, dth, sigma), A.jpprod(x, dth)])
    assert np.abs(rhs).max() > 0
    want = scipy.linalg.solve(K, rhs)
    kkt = ScipyKKT(K)
    dx, dy = parameter_step(HostParamModel(core, blob), kkt, torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(dth), obj_weight=sigma)
    assert kkt.calls == 1 and dx.shape == (om.nvar,) and dy.shape == (om.ncon,)
    got = np.concatenate([dx.numpy(), dy.numpy()])
    err = np.abs(got - want).max() / max(1.0, np.abs(want).max())
    print(name, seed, "relative error", err, "max |step|", np.abs(want).max())
    assert err <= TOL


def _attached(m):
    from infiniteexamodels.jl_amd.backend import ExaTranscriptionBackend
    be = ExaTranscriptionBackend.__new__(ExaTranscriptionBackend)
    be.data = transcribe.ExaMappingData()
    be.core = transcribe.exa_core(m, be.data)
    be._inf_model = m
    return be


def test_parameter_direction_is_what_update_would_write(built):
    m, (P1, P2) = cases.rosenbrock()
    be = _attached(m)
    th0 = np.array(be.core.theta, copy=True)
    d = be.parameter_direction(P2, 3.5)
    np.testing.assert_array_equal(be.core.theta, th0)        # θ untouched
    assert P2.value == 1.0
    assert be.update_parameter_value(P2, 3.5)
    np.testing.assert_array_equal(d, np.asarray(be.core.theta) - th0)
    assert d.shape == th0.shape and np.count_nonzero(d) == 1

    m, (pf1, pf2) = cases.pfun()
    be = _attached(m)
    th0 = np.array(be.core.theta, copy=True)
    f_old = pf2.func
    new = lambda t, s: np.cos(t) * s - 0.3   # noqa: E731
    d = be.parameter_direction(pf2, new)
    np.testing.assert_array_equal(be.core.theta, th0)
    assert pf2.func is f_old
    assert be.update_parameter_value(pf2, new)
    np.testing.assert_array_equal(d, np.asarray(be.core.theta) - th0)
    par = be.data.param_mappings[pf2]
    assert np.count_nonzero(d) == par.length and not d[:par.offset].any()
    with pytest.raises(KeyError):
        be.parameter_direction(object(), 1.0)
