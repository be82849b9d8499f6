"""The operator-domain sweep of test_op_domain.py on the device: both models (cases_op_domain.py) through
``ExaModel(device=0)`` in both code shapes, into NaN-poisoned output buffers, against the 50-digit mpmath reference
(op_domain_reference.py).  This is where ocml's pow, cbrt, log1p, atanh, exp2 and the sincos pairing at arguments up to 1e15
meet something better than glibc at one point.

Per output element: the hard bound |got - ref| <= 1e-10·|ref| (no floor, no exception) and the sharp bound
|got - ref| <= max(8·e_oracle, 32·2⁻⁵³·|ref|), e_oracle being the oracle's own error at the same element, computed here.  The
margin of 8: glibc is correctly rounded or within 1 ulp where ocml documents up to 2 ulp, and a derivative chains up to three
such values; it comes from the reference and the oracle, never from the device's numbers.  An operator that meets the hard
bound but not the sharp one is either rewritten or named in SHARP_EXCEPTIONS (at most 3) with its measured ulp and cause.

The derived programs (lagrad, kktprod, the scaled and the θ programs) share unary() and binary() and are pinned bitwise to
compositions of these calls by their own tests: they are not swept again."""
import numpy as np
import pytest

import op_domain_reference as R

pytestmark = pytest.mark.gpu

MODELS = ("unary_sweep", "binary_sweep")
# operator -> (measured error in ulp, cause); the hard bound has no exceptions
SHARP_EXCEPTIONS = {}
assert len(SHARP_EXCEPTIONS) <= 3


class GpuEval(R.Evaluator):
    """ExaModel's entry points as numpy arrays, every output written into a NaN-poisoned buffer"""
    name = "gpu"

    def __init__(self, om, gm, torch):
        super().__init__(om)
        self.gm, self.torch = gm, torch

    def _d(self, a):
        return self.torch.tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")

    def _nan(self, n):
        return self.torch.full((n,), float("nan"), device="cuda", dtype=self.torch.float64)

    def obj(self, x): return self.gm.obj(self._d(x))
    def cons(self, x): return self.gm.cons(self._d(x), self._nan(self.om.ncon)).cpu().numpy()
    def grad(self, x): return self.gm.grad(self._d(x), self._nan(self.om.nvar)).cpu().numpy()
    def jac_coord(self, x): return self.gm.jac_coord(self._d(x), self._nan(self.om.nnzj)).cpu().numpy()
    def hess_coord(self, x, y, w): return self.gm.hess_coord(self._d(x), self._d(y), self._nan(self.om.nnzh), obj_weight=w).cpu().numpy()
    def jprod(self, x, v): return self.gm.jprod(self._d(x), self._d(v), self._nan(self.om.ncon)).cpu().numpy()
    def jtprod(self, x, v): return self.gm.jtprod(self._d(x), self._d(v), self._nan(self.om.nvar)).cpu().numpy()
    def hprod(self, x, y, v, w): return self.gm.hprod(self._d(x), self._d(y), self._d(v), self._nan(self.om.nvar), obj_weight=w).cpu().numpy()
    def set_theta(self, value): self.gm.set_parameter(0, [value])


@pytest.fixture(scope="module")
def torch_cuda(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture
def on_gpu(torch_cuda, grid_mode):
    """model name -> (case, evaluator on the device) in the code shape of `grid_mode`; the handles are closed afterwards"""
    from infiniteexamodels.jl_amd.model import ExaModel
    opened = []

    def make(model):
        c = R.sweep_case(model)
        gm = ExaModel(c.core, device=0, blob=c.blob)
        opened.append(gm)
        om = c.oe.om
        assert (gm.meta.nvar, gm.meta.ncon, gm.meta.nnzj, gm.meta.nnzh) == (om.nvar, om.ncon, om.nnzj, om.nnzh)
        ev = GpuEval(om, gm, torch_cuda)
        for got, want in zip(gm.jac_structure() + gm.hess_structure(), (ev.jr, ev.jc, ev.hr, ev.hc)):
            assert np.array_equal(got, want)
        return c, ev
    yield make
    for gm in opened:
        gm.close()


def _report(bad):
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:60])


@pytest.mark.parametrize("model", MODELS)
def test_kernels_over_the_domain(model, on_gpu):
    c, ev = on_gpu(model)
    out = R.outputs(ev, c.ref, c.x, c.y, c.v, c.vc)
    for op, d in sorted(R.worst_by_owner(model, c.ref, out).items()):      # the figures, before anything is asserted
        print(f"{model} {op}: " + " ".join(f"{k}={e * 2.0 ** 53:.1f}u" for k, e in d.items()))
    _report(R.check(model, c.ref, out, c.regions, c.e_oracle, exceptions=tuple(SHARP_EXCEPTIONS)))


def test_runtime_exponent(on_gpu):
    c, ev = on_gpu("binary_sweep")
    _report(R.theta_failures(c, ev))


@pytest.mark.parametrize("model", MODELS)
def test_special_points(model, on_gpu):
    c, ev = on_gpu(model)
    _report(R.special_failures(c, ev))


def test_runtime_exponent_at_zero_base_is_nan_in_both(on_gpu):
    c, ev = on_gpu("binary_sweep")
    _report(R.theta_zero_base_failures(c, ev))


@pytest.mark.parametrize("op,value", R.BAD_LANES)
def test_one_bad_lane_stays_one_bad_lane(op, value, on_gpu):
    c, ev = on_gpu("unary_sweep")
    _report(R.bad_lane_failures(c, ev, op, value))
