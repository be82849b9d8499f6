"""sensitivity.value_gradient / value_hessian_product(s) — second-order θ sensitivities of the value function
φ(θ) = L(x*(θ), y*(θ), θ) — on the CPU.

The generated kernels compiled for the host behind ExaModel's method names, through the dense stub `kkt` of
tests/test_parameter_step.py (scipy's LU of K assembled from the oracle, δw = δc = 1e-2, symmetric, cond ≤ 1e6), against
    L_θθ·δθ − Gᵀ·(K⁻¹·(G·δθ)),      G = [∂²L/∂x∂θ ; ∂c/∂θ],
assembled from the autograd witness's products (hppprod, hpprod, jpprod, hptprod, jptprod) and numpy.linalg.solve.  Both
sides are sums of products rounded independently: the bound is 1e-10 times the sum of the absolute values of every
addend — per entry j of θ, |L_θθ·δθ|_j + Σ_i |G_ij|·|K⁻¹Gδθ|_i (the convention of tests/test_parameter_gradient.py)."""
import numpy as np
import pytest

from emu_theta2 import EmulatedTheta2Model
from infiniteexamodels.jl_amd.sensitivity import value_gradient, value_hessian_product, value_hessian_products
from pyoracle import OracleModel
from test_kkt import host_kkt
from test_parameter_gradient import HostAdjointModel
from test_parameter_step import ScipyKKT, _cores
from theta2_witness import WitnessTheta2

TOL = 1e-10


class HostTheta2Model(HostAdjointModel):
    """... plus hppprod (its own program)"""

    def __init__(self, core, blob):
        super().__init__(core, blob)
        self.th2 = EmulatedTheta2Model(core, blob)

    def hppprod(self, x, y, w, obj_weight=1.0, out=None):
        import torch
        v = torch.from_numpy(self.th2.hppprod(x.numpy(), y.numpy(), w.numpy(), obj_weight).copy())
        return v if out is None else out.copy_(v)


_cache = {}


def _system(name, seed):
    if (name, seed) not in _cache:
        core = _cores()[name]()
        blob = core.to_blob()
        om = OracleModel(blob)
        rng = np.random.default_rng(60 + seed)
        x = om.x0 + 0.1 * rng.standard_normal(om.nvar)
        y = rng.standard_normal(om.ncon)
        sigma = 1.0 if seed == 0 else 0.6
        K = host_kkt(om, x, y, np.zeros(om.nvar), 1e-2, 1e-2, w=sigma).toarray()
        assert np.abs(K - K.T).max() == 0.0 and np.linalg.cond(K) <= 1e6
        A = WitnessTheta2(core)
        absG = np.abs(np.stack([np.concatenate([A.hpprod(x, y, e, sigma), A.jpprod(x, e)]) for e in np.eye(om.npar)], axis=1))
        _cache[name, seed] = (om, HostTheta2Model(core, blob), A, K, absG, x, y, sigma)
    return _cache[name, seed]


def _want(A, K, absG, x, y, sigma, dth):
    """the witness's φ''·δθ and, per entry, the sum of the absolute values of its addends"""
    direct = A.hppprod(x, y, dth, sigma)
    sol = np.linalg.solve(K, np.concatenate([A.hpprod(x, y, dth, sigma), A.jpprod(x, dth)]))
    return direct - A.gt_lambda(x, y, sol, sigma), np.abs(direct) + absG.T @ np.abs(sol)


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("name", ["quadrotor_11", "pfun"])
def test_value_hessian_product_matches_the_dense_answer(name, seed, built):
    import torch
    om, hm, A, K, absG, x, y, sigma = _system(name, seed)
    rng = np.random.default_rng(70 + seed)
    w, u = rng.standard_normal(om.npar), rng.standard_normal(om.npar)
    xt, yt = torch.from_numpy(x), torch.from_numpy(y)
    kkt = ScipyKKT(K)
    got_w = value_hessian_product(hm, kkt, xt, yt, torch.from_numpy(w), obj_weight=sigma)
    assert kkt.calls == 1 and tuple(got_w.shape) == (om.npar,)
    got_w = got_w.numpy()
    want_w, scale_w = _want(A, K, absG, x, y, sigma, w)
    print(name, seed, "max |want|", np.abs(want_w).max(), "worst error / scale", (np.abs(got_w - want_w) / np.maximum(scale_w, 1e-300)).max())
    assert np.abs(want_w).max() > 0 and np.abs(A.hppprod(x, y, w, sigma)).max() > 0
    assert (np.abs(got_w - want_w) <= TOL * scale_w).all()
    # φ'' is symmetric: u·(φ''w) == w·(φ''u)
    got_u = value_hessian_product(hm, ScipyKKT(K), xt, yt, torch.from_numpy(u), obj_weight=sigma).numpy()
    _, scale_u = _want(A, K, absG, x, y, sigma, u)
    lhs, rhs = float(u @ got_w), float(w @ got_u)
    assert abs(lhs - rhs) <= TOL * float(np.abs(u) @ scale_w + np.abs(w) @ scale_u), (lhs, rhs)


@pytest.mark.parametrize("name", ["quadrotor_11", "pfun"])
def test_products_are_one_solve_and_equal_the_single_ones(name, built):
    import torch
    om, hm, A, K, absG, x, y, sigma = _system(name, 1)
    D = np.random.default_rng(79).standard_normal((om.npar, 3))
    xt, yt = torch.from_numpy(x), torch.from_numpy(y)

    shapes = []

    class Recording(ScipyKKT):
        def solve(self, rhs):
            shapes.append(tuple(rhs.shape))
            return super().solve(rhs)
    kkt = Recording(K)
    many = value_hessian_products(hm, kkt, xt, yt, torch.from_numpy(D), obj_weight=sigma)
    assert kkt.calls == 1 and shapes == [(om.nvar + om.ncon, 3)] and tuple(many.shape) == (om.npar, 3)
    for j in range(3):
        one = value_hessian_product(hm, ScipyKKT(K), xt, yt, torch.from_numpy(D[:, j].copy()), obj_weight=sigma).numpy()
        _, scale = _want(A, K, absG, x, y, sigma, D[:, j])
        assert (np.abs(many[:, j].numpy() - one) <= TOL * scale).all(), j      # (scipy's multi-column LU solve may round a column differently)
    as_list = value_hessian_products(hm, ScipyKKT(K), xt, yt, [D[:, j].copy() for j in range(3)], obj_weight=sigma)
    assert np.array_equal(as_list.numpy(), many.numpy())
    with pytest.raises(ValueError):
        value_hessian_products(hm, kkt, xt, yt, torch.from_numpy(D[:, 0].copy()))


@pytest.mark.parametrize("name", ["quadrotor_11", "pfun"])
def test_value_gradient_is_jptprod(name, built):
    import torch
    om, hm, A, K, absG, x, y, sigma = _system(name, 0)
    xt, yt = torch.from_numpy(x), torch.from_numpy(y)
    g = value_gradient(hm, xt, yt, obj_weight=0.8).numpy()
    assert np.array_equal(g, hm.jptprod(xt, yt, obj_weight=0.8).numpy())
    want = A.jptprod(x, y, 0.8)
    assert np.abs(g - want).max() <= TOL * max(1.0, np.abs(want).max())
