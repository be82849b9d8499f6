"""sensitivity.parameter_jacobian without a device: the gather plan (duplicates, repeated and unused columns, refusals)
and the formula itself — a stub model whose COO blocks come from dense random matrices, a dense NumPy solve for ``kkt`` —
against −K⁻¹·G[:, cols] computed densely."""
import types

import numpy as np
import pytest
import torch

from infiniteexamodels.jl_amd import sensitivity as S


def coo_of(dense, rng, dup=0.3):
    """COO triplets of a dense block in shuffled order, a share of the entries split into two addends"""
    r, c = np.nonzero(dense)
    v = dense[r, c]
    split = rng.random(len(r)) < dup
    part = rng.standard_normal(int(split.sum()))
    r = np.concatenate([r, r[split]]); c = np.concatenate([c, c[split]])
    v = np.concatenate([v, part])
    v[:len(split)][split] -= part
    p = rng.permutation(len(r))
    return r[p].astype(np.int64), c[p].astype(np.int64), v[p]


class StubModel:
    def __init__(self, nvar, ncon, npar, seed=0):
        rng = np.random.default_rng(seed)
        self.meta = types.SimpleNamespace(nvar=nvar, ncon=ncon, npar=npar)
        self.Hxp = rng.standard_normal((nvar, npar)) * (rng.random((nvar, npar)) < 0.3)
        self.Jp = rng.standard_normal((ncon, npar)) * (rng.random((ncon, npar)) < 0.3)
        self.Hxp[:, 2] = 0.0; self.Jp[:, 2] = 0.0          # a θ entry nothing depends on
        self.xp, self.jp = coo_of(self.Hxp, rng), coo_of(self.Jp, rng)
        self.calls = {"hessp_coord": 0, "jacp_coord": 0}

    def hessxp_structure(self, base=0):
        return self.xp[0] + base, self.xp[1] + base

    def jacp_structure(self, base=0):
        return self.jp[0] + base, self.jp[1] + base

    def hessp_coord(self, x, y, obj_weight=1.0, vals_xp=None, vals_pp=None):
        self.calls["hessp_coord"] += 1
        assert vals_pp is False      # the θθ block is not wanted
        vals_xp.copy_(torch.tensor(obj_weight * self.xp[2]))
        return vals_xp, vals_pp

    def jacp_coord(self, x, vals=None):
        self.calls["jacp_coord"] += 1
        vals.copy_(torch.tensor(self.jp[2]))
        return vals


class DenseKKT:
    def __init__(self, n, seed=1):
        a = np.random.default_rng(seed).standard_normal((n, n))
        self.K = a + a.T + 2 * n * np.eye(n)
        self.rhs = []

    def solve(self, rhs):
        self.rhs.append(rhs.clone())
        return torch.tensor(np.linalg.solve(self.K, rhs.numpy()))


def test_plan_merges_duplicates_in_a_fixed_order():
    # Hxθ: (row 0, θ1) three times at COO positions 0, 2, 3; (row 1, θ0) once; Jθ: (row 0, θ1) twice
    xr, xc = np.array([0, 1, 0, 0]), np.array([1, 0, 1, 1])
    jr, jc = np.array([0, 0]), np.array([1, 1])
    p = S.ParameterJacobianPlan((xr, xc), (jr, jc), nvar=2, ncon=1, npar=3, theta_cols=[1, 0, 1])
    # destinations k·3 + row: k = 0 and k = 2 take θ1, k = 1 takes θ0
    np.testing.assert_array_equal(p.dest, [0, 2, 4, 6, 8])
    np.testing.assert_array_equal(p.seg, [0, 3, 5, 6, 9, 11])
    np.testing.assert_array_equal(p.perm, [0, 2, 3, 4, 5, 1, 0, 2, 3, 4, 5])      # duplicates keep their COO order
    vals = torch.tensor([1.0, 10.0, 2.0, 4.0, 0.5, 0.25])
    rhs = p.rhs(None, vals)
    np.testing.assert_array_equal(rhs.numpy(), -np.array([[7.0, 0.0, 0.75], [0.0, 10.0, 0.0], [7.0, 0.0, 0.75]]))
    again = S.ParameterJacobianPlan((xr, xc), (jr, jc), 2, 1, 3, [1, 0, 1])
    for a in ("dest", "seg", "perm"):
        np.testing.assert_array_equal(getattr(p, a), getattr(again, a))


def test_plan_refusals():
    s = (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
    with pytest.raises(ValueError):
        S.ParameterJacobianPlan(s, s, 2, 1, 3, [])
    with pytest.raises(IndexError):
        S.ParameterJacobianPlan(s, s, 2, 1, 3, [0, 3])
    with pytest.raises(IndexError):
        S.ParameterJacobianPlan(s, s, 2, 1, 3, [-1])
    with pytest.raises(TypeError):
        S.ParameterJacobianPlan(s, s, 2, 1, 3, [0.5])
    p = S.ParameterJacobianPlan(s, s, 2, 1, 3, [2])          # nothing depends on θ: a zero right-hand side
    assert p.rhs(None, torch.zeros(0, dtype=torch.float64)).abs().max() == 0


@pytest.mark.parametrize("sigma", [1.0, -0.5])
def test_the_formula_against_a_dense_solve(sigma):
    nvar, ncon, npar = 9, 5, 6
    m, kkt = StubModel(nvar, ncon, npar), DenseKKT(nvar + ncon)
    cols = [4, 0, 2, 4, 5]
    x, y = torch.zeros(nvar, dtype=torch.float64), torch.zeros(ncon, dtype=torch.float64)
    dX, dY = S.parameter_jacobian(m, kkt, x, y, cols, obj_weight=sigma)
    G = np.vstack([sigma * m.Hxp, m.Jp])
    want = -np.linalg.solve(kkt.K, G[:, cols])
    assert dX.shape == (nvar, len(cols)) and dY.shape == (ncon, len(cols))
    got = np.vstack([dX.numpy(), dY.numpy()])
    # the right-hand side differs from −G[:, cols] by the rounding of the split duplicates only; the solve is the same
    assert np.abs(kkt.rhs[0].numpy() + G[:, cols]).max() <= 8 * 2.0 ** -52 * np.abs(G).max() * 4
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    np.testing.assert_array_equal(got[:, 0], got[:, 3])       # the repeated index
    assert np.abs(got[:, 2]).max() == 0                       # the θ entry nothing depends on
    assert len(kkt.rhs) == 1 and kkt.rhs[0].shape == (nvar + ncon, len(cols))      # ONE solve, 2-D
    assert m.calls == {"hessp_coord": 1, "jacp_coord": 1}
    S.parameter_jacobian(m, kkt, x, y, cols, obj_weight=sigma)
    assert len(m.__dict__["_parameter_jacobian_plans"]) == 1   # the plan is built once per (model, cols)


def test_parameter_columns_are_what_gradient_values_cuts_by(built):
    import cases
    from test_parameter_step import _attached
    m, (P1, P2) = cases.rosenbrock()
    be = _attached(m)
    c1, c2 = be.parameter_columns(P1), be.parameter_columns(P2)
    assert c1.dtype == np.int64 and len(c1) == len(c2) == 1 and c1[0] != c2[0]
    g = np.arange(be.core.npar, dtype=np.float64) + 10.0
    assert be.parameter_gradient_values(P2, g) == g[c2[0]]
    m, (pf1, pf2) = cases.pfun()
    be = _attached(m)
    cols = be.parameter_columns(pf2)
    g = np.random.default_rng(0).standard_normal(be.core.npar)
    np.testing.assert_array_equal(be.parameter_gradient_values(pf2, g).reshape(-1, order="F"), g[cols])
    assert not set(cols) & set(be.parameter_columns(pf1))
    with pytest.raises(KeyError):
        be.parameter_columns("not a parameter")
