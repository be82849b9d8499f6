"""sensitivity.parameter_gradient(s) — the adjoint mode — and ExaTranscriptionBackend.parameter_gradient_values on the CPU.

The adjoint answer is checked against the FORWARD mode that already exists: for any direction δθ and any g = [gx; gy],
parameter_gradient(gx, gy)·δθ must equal gx·dx + gy·dy with (dx, dy) = parameter_step(δθ) — both through the same dense
stub `kkt` (scipy's LU of K assembled from the oracle, as in tests/test_parameter_step.py, δw = δc = 1e-2, symmetric, cond
≤ 1e6), the generated kernels compiled for the host behind ExaModel's method names.  The two sides are sums of products
rounded independently: the bound is 1e-10 times the sum of the absolute values of every addend on either side."""
import numpy as np
import pytest

from emu_adjoint import EmulatedAdjointModel
from infiniteexamodels.jl_amd.sensitivity import parameter_gradient, parameter_gradients, parameter_step
from pyoracle import OracleModel
from test_kkt import host_kkt
from test_parameter_step import HostParamModel, ScipyKKT, _attached, _cores

TOL = 1e-10


class HostAdjointModel(HostParamModel):
    """... plus hptprod (its own program) and jptprod"""

    def __init__(self, core, blob):
        super().__init__(core, blob)
        self.adj = EmulatedAdjointModel(core, blob)

    def hptprod(self, x, y, u, obj_weight=1.0, out=None):
        import torch
        v = torch.from_numpy(self.adj.hptprod(x.numpy(), y.numpy(), u.numpy(), obj_weight).copy())
        return v if out is None else out.copy_(v)

    def jptprod(self, x, y, obj_weight=1.0, out=None):
        import torch
        v = torch.from_numpy(self.em.jptprod(x.numpy(), y.numpy(), obj_weight).copy())
        return v if out is None else out.copy_(v)


_cache = {}


def _system(name, seed):
    if (name, seed) not in _cache:
        core = _cores()[name]()
        blob = core.to_blob()
        om = OracleModel(blob)
        rng = np.random.default_rng(40 + seed)
        x = om.x0 + 0.1 * rng.standard_normal(om.nvar)
        y = rng.standard_normal(om.ncon)
        sigma = 1.0 if seed == 0 else 0.6
        K = host_kkt(om, x, y, np.zeros(om.nvar), 1e-2, 1e-2, w=sigma).toarray()
        assert np.abs(K - K.T).max() == 0.0 and np.linalg.cond(K) <= 1e6
        _cache[name, seed] = (om, HostAdjointModel(core, blob), K, x, y, sigma, rng)
    return _cache[name, seed]


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("name", ["quadrotor_11", "pfun"])
def test_adjoint_gradient_matches_the_forward_step(name, seed, built):
    import torch
    om, hm, K, x, y, sigma, rng = _system(name, seed)
    gx, gy = rng.standard_normal(om.nvar), rng.standard_normal(om.ncon)
    dth = 0.1 * rng.standard_normal(om.npar)
    dq = rng.standard_normal(om.npar)
    xt, yt = torch.from_numpy(x), torch.from_numpy(y)
    kkt = ScipyKKT(K)
    grad = parameter_gradient(hm, kkt, xt, yt, torch.from_numpy(gx), torch.from_numpy(gy), obj_weight=sigma, dq_dtheta=torch.from_numpy(dq))
    assert kkt.calls == 1 and grad.shape == (om.npar,)
    dx, dy = parameter_step(hm, ScipyKKT(K), xt, yt, torch.from_numpy(dth), obj_weight=sigma)
    dx, dy, grad = dx.numpy(), dy.numpy(), grad.numpy()
    lhs = float((grad - dq) @ dth)
    rhs = float(gx @ dx + gy @ dy)
    scale = float(np.abs(grad - dq) @ np.abs(dth) + np.abs(gx) @ np.abs(dx) + np.abs(gy) @ np.abs(dy))
    print(name, seed, lhs, rhs, abs(lhs - rhs) / scale)
    assert abs(rhs) > 0 and abs(lhs - rhs) <= TOL * scale
    # gy = None means zeros, dq_dtheta = None means zeros
    g0 = parameter_gradient(hm, ScipyKKT(K), xt, yt, torch.from_numpy(gx), obj_weight=sigma).numpy()
    lhs0, rhs0 = float(g0 @ dth), float(gx @ dx)
    assert abs(lhs0 - rhs0) <= TOL * float(np.abs(g0) @ np.abs(dth) + np.abs(gx) @ np.abs(dx))


@pytest.mark.parametrize("name", ["quadrotor_11", "pfun"])
def test_gradients_are_one_solve_and_equal_the_single_ones(name, built):
    import torch
    om, hm, K, x, y, sigma, rng = _system(name, 1)
    G = np.random.default_rng(77).standard_normal((om.nvar + om.ncon, 4))
    DQ = np.random.default_rng(78).standard_normal((om.npar, 4))
    xt, yt = torch.from_numpy(x), torch.from_numpy(y)
    kkt = ScipyKKT(K)
    many = parameter_gradients(hm, kkt, xt, yt, torch.from_numpy(G), obj_weight=sigma, dq_dtheta=torch.from_numpy(DQ))
    assert kkt.calls == 1 and tuple(many.shape) == (om.npar, 4)
    for j in range(4):
        one = parameter_gradient(hm, ScipyKKT(K), xt, yt, torch.from_numpy(G[:om.nvar, j].copy()), torch.from_numpy(G[om.nvar:, j].copy()),
                                 obj_weight=sigma, dq_dtheta=torch.from_numpy(DQ[:, j].copy())).numpy()
        err = np.abs(many[:, j].numpy() - one).max() / max(1.0, np.abs(one).max())
        assert err <= TOL, (j, err)         # (scipy's multi-column LU solve may round a column differently from a single one)
    with pytest.raises(ValueError):
        parameter_gradients(hm, kkt, xt, yt, torch.from_numpy(G[:, 0].copy()))
    with pytest.raises(ValueError):
        parameter_gradients(hm, kkt, xt, yt, torch.from_numpy(G[:-1]))


def test_gradient_values_invert_parameter_direction(built):
    import cases
    m, (P1, P2) = cases.rosenbrock()
    be = _attached(m)
    d = be.parameter_direction(P2, 3.5)
    v = be.parameter_gradient_values(P2, d)
    assert isinstance(v, float) and v == 3.5 - P2.value
    assert be.parameter_gradient_values(P1, d) == 0.0

    m, (pf1, pf2) = cases.pfun()
    be = _attached(m)
    new = lambda t, s: np.cos(t) * s - 0.3   # noqa: E731
    d = be.parameter_direction(pf2, new)
    par = be.data.param_mappings[pf2]
    got = be.parameter_gradient_values(pf2, d)
    assert got.shape == tuple(par.size) and got.ndim == 2
    from infiniteexamodels.jl_amd import transcribe
    old = np.asarray(transcribe._eval_over_supports(pf2.func, m, pf2.group_idxs, par.size), dtype=np.float64)
    want = np.asarray(transcribe._eval_over_supports(new, m, pf2.group_idxs, par.size), dtype=np.float64) - old
    np.testing.assert_array_equal(got, want.reshape(par.size))
    np.testing.assert_array_equal(got.reshape(-1, order="F"), d[par.offset:par.offset + par.length])
    assert not be.parameter_gradient_values(pf1, d).any() and be.parameter_gradient_values(pf1, d).shape == tuple(be.data.param_mappings[pf1].size)
    with pytest.raises(KeyError):
        be.parameter_gradient_values(object(), d)
    with pytest.raises(ValueError):
        be.parameter_gradient_values(pf2, d[:-1])
