"""Every operator of the table the kernels take their arithmetic from (Sweep::unary / Sweep::binary of csrc/iem_codegen.cpp,
restated by un_eval / bin_partials of oracle/iem_oracle.c) over its whole domain — positive and negative, tiny and large
arguments, the domain edges — against 50-digit mpmath references (op_domain_reference.py), on the CPU: the oracle, and the
GENERATED kernels' text run by emu.EmulatedModel in both code shapes, which pins the generator's table without a GPU.  The GPU
twin is test_gpu_op_domain.py.

Per output element (cons, grad, jac_coord, hess_coord with random y and σ = 0.7; jprod / jtprod / hprod relative to Σ|addend|,
obj relative to Σ|term|):

  hard   |got - ref| <= 1e-10·|ref| — the project's bar, purely relative, no floor, no exception;
  sharp  |got - ref| <= max(8·e_oracle, 32·2⁻⁵³·|ref|), e_oracle the oracle's own error at the same element.

Then the special points (±0, the domain ends, constant exponents at a = 0: finite limits exactly, everything else class for
class the oracle's), the run-time exponent θ₀, and one item moved out of its domain.

The derived programs (lagrad, kktprod, the scaled and the θ programs) share unary() and binary() and are pinned bitwise to
compositions of these calls by their own tests: they are not swept again."""
import numpy as np
import pytest

import cases_op_domain as D
import op_domain_reference as R
from emu import EmulatedModel

MODELS = ("unary_sweep", "binary_sweep")


@pytest.fixture(scope="module")
def case(built):
    return R.sweep_case


def _emulated(c):
    return R.EmuEval(c.oe.om, EmulatedModel(c.core, c.blob))


def _report(bad):
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:60])


@pytest.mark.parametrize("model", MODELS)
def test_models_have_the_shape_the_sweep_needs(model, case):
    c = case(model)
    om = c.oe.om
    if model == "unary_sweep":
        assert len(D.OPS) == 39 and (om.nvar, om.ncon, om.n_templates) == (40 * D.N, 78 * D.N, 117)
    else:
        assert (om.nvar, om.ncon, om.npar) == (2 * len(D.FORMS) * D.N, len(D.FORMS) * D.N, 1)
    assert D.N == 320 and np.isfinite(c.x).all()
    for what, (got, ref, scale) in c.out_oracle.items():
        assert np.isfinite(ref).all() and np.isfinite(np.asarray(got)).all(), f"{what}: a region outside the domain"
    for regs in c.regions.values():      # every region of every operator is met by more than one wavefront's worth of draws
        assert min(regs.count(r) for r in set(regs)) >= D.N // 8


@pytest.mark.parametrize("model", MODELS)
def test_oracle_meets_the_bar_over_the_domain(model, case):
    c = case(model)
    _report(R.check(model, c.ref, c.out_oracle, c.regions))


@pytest.mark.parametrize("model", MODELS)
def test_emulated_kernels_over_the_domain(model, case, grid_mode):
    c = case(model)
    _report(R.sweep_failures(c, _emulated(c)))


def test_oracle_runtime_exponent(case):
    c = case("binary_sweep")
    _report(R.theta_failures(c, c.oe, sharp=False))


def test_emulated_runtime_exponent(case, grid_mode):
    c = case("binary_sweep")
    _report(R.theta_failures(c, _emulated(c)))


@pytest.mark.parametrize("model", MODELS)
def test_oracle_special_points(model, case):
    c = case(model)
    _report(R.special_failures(c, c.oe))


@pytest.mark.parametrize("model", MODELS)
def test_emulated_special_points(model, case, grid_mode):
    c = case(model)
    _report(R.special_failures(c, _emulated(c)))


def test_runtime_exponent_at_zero_base_is_nan_in_both(case, grid_mode):
    c = case("binary_sweep")
    _report(R.theta_zero_base_failures(c, _emulated(c)))


@pytest.mark.parametrize("op,value", R.BAD_LANES)
def test_one_bad_lane_stays_one_bad_lane(op, value, case, grid_mode):
    c = case("unary_sweep")
    _report(R.bad_lane_failures(c, _emulated(c), op, value))
