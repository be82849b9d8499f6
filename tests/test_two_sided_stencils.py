"""Evaluation of stencils that reach to the RIGHT of their support: forward differences (canonical slot at i, neighbour
at i + 1) and central differences (neighbours on both sides, no slot at i for the differentiated state) —
/root/reference/src/transform.jl:535 passes any finite-difference method to `derivative_expr_data`; the heat workload adds
the nested second derivative (transform.jl:141).  Oracle ≡ autograd ≡ host-compiled generated kernels, at the tolerances
of tests/test_oracle_autodiff.py and tests/test_codegen_emulation.py; and the scatter kinds come out without a
floating-point atomic, as the generator's file header promises for backward differences."""
import os
import re

import numpy as np
import pytest

import cases_two_sided as C2
from emu import EmulatedModel
from helpers import TorchModel, coo_to_dense, lower_to_full
from pyoracle import OracleModel

NAMES = list(C2.MODELS)


def _rel(a, b):
    return 0.0 if len(b) == 0 else float(np.abs(a - b).max() / max(1e-300, np.abs(b).max()))


@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_autograd(name, built):
    core = C2.build_core(name)
    om = OracleModel(core.to_blob())
    x, y = C2.eval_point(om)
    f, c, g, J, H = TorchModel(core).dense(x, y, 0.7)
    assert abs(om.obj(x) - f) <= 1e-12 * max(1.0, abs(f))
    np.testing.assert_allclose(om.cons(x), c, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(om.grad(x), g, rtol=1e-12, atol=1e-12)
    r, cc = om.jac_structure()
    np.testing.assert_allclose(coo_to_dense(r, cc, om.jac_coord(x), (om.ncon, om.nvar)), J, rtol=1e-12, atol=1e-12)
    r, cc = om.hess_structure()
    Ho = lower_to_full(coo_to_dense(r, cc, om.hess_coord(x, y, 0.7), (om.nvar, om.nvar)))
    np.testing.assert_allclose(Ho, H, rtol=1e-11, atol=1e-11 * max(1.0, np.abs(H).max()))
    vc = np.random.default_rng(9).standard_normal(om.ncon)
    np.testing.assert_allclose(om.jtprod(x, vc), J.T @ vc, rtol=1e-11, atol=1e-11)


@pytest.mark.parametrize("name", NAMES)
def test_emulated_kernels_match_oracle(name, grid_mode):
    core = C2.build_core(name)
    blob = core.to_blob()
    om = OracleModel(blob)
    x, y = C2.eval_point(om)
    em = EmulatedModel(core, blob)
    assert abs(em.obj(x) - om.obj(x)) <= 1e-12 * max(1.0, abs(om.obj(x)))
    assert _rel(em.cons(x), om.cons(x)) <= 1e-14
    assert _rel(em.grad(x), om.grad(x)) <= 1e-14
    j = em.jac_coord(x, om.nnzj)
    h = em.hess_coord(x, y, 0.7, om.nnzh)
    assert not np.isnan(j).any() and not np.isnan(h).any(), "every output slot must be written"
    assert _rel(j, om.jac_coord(x)) <= 1e-14
    assert _rel(h, om.hess_coord(x, y, 0.7)) <= 1e-14
    rng = np.random.default_rng(5)
    v, vc = rng.standard_normal(om.nvar), rng.standard_normal(om.ncon)
    assert _rel(em.jprod(x, v), om.jprod(x, v)) <= 1e-13
    assert _rel(em.jtprod(x, vc), om.jtprod(x, vc)) <= 1e-13
    assert _rel(em.hprod(x, y, v, 0.7), om.hprod(x, y, v, 0.7)) <= 1e-13


def _float_atomic_calls():
    """What the generator writes for a floating-point atomic, read from the sources themselves: the `iem_*` helpers of the
    device header whose body calls atomicAdd / unsafeAtomicAdd, as far as csrc/iem_codegen.cpp emits calls to them, and
    any such call the generator writes directly."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "infiniteexamodels.jl_amd", "csrc")
    hdr = open(os.path.join(csrc, "iem_device.h")).read()
    gen = open(os.path.join(csrc, "iem_codegen.cpp")).read()
    helpers = set()
    for m in re.finditer(r"void (iem_\w+)\(double \*__restrict__ \w+[^{]*\{([^}]*)\}", hdr):
        if re.search(r"\b(unsafeA|a)tomicAdd\(", m.group(2)):
            helpers.add(m.group(1))
    emitted = {h for h in helpers if h + "(" in gen}
    assert emitted == {"iem_grad_atomic", "iem_grad_wave_uniform"}, emitted   # the calls tests/test_codegen_emulation.py counts, too
    direct = [s for s in ("atomicAdd(", "unsafeAtomicAdd(") if s in gen]
    return sorted(emitted), direct


@pytest.mark.parametrize("name", NAMES)
def test_scatter_kinds_hold_no_float_atomic(name, grid_mode):
    """grad! / jtprod! / hprod! of forward and central models under default options: every entry gets one exclusive store
    (pull_neighbours handles shifts of either sign), none an atomic."""
    from infiniteexamodels.jl_amd import lib as iemlib
    helpers, direct = _float_atomic_calls()
    src, _ = iemlib.emit_source(C2.build_core(name).to_blob())
    generated = src[src.index("#endif  // IEM_DEVICE_H"):]
    kinds = set(re.findall(r"void (iem_(?:grad|jtprod|hprod)\w*)\(", generated))
    assert all(any(k.startswith(p) for k in kinds) for p in ("iem_grad", "iem_jtprod", "iem_hprod")), kinds
    for call in [h + "(" for h in helpers] + direct:
        assert call not in generated, (name, call)


def test_chain_kkt_analysis_is_pinned(built):
    """`iem_kkt_analyse_blob` (host analysis, no device) on the new models — the solver itself is not extended, what it
    does today is pinned.  Central differences couple support i with i ± 1 through rows at i, which the chain takes as
    pairs of supports with reach 2; forward differences stay at reach 1.  The heat workload is a chain along t (one block
    per time support holding every x); left to pick the group itself the analysis refuses it and names the coupling the x
    stencil creates."""
    from infiniteexamodels.jl_amd import lib as iemlib
    central = iemlib.kkt_analyse_blob(C2.build_core("central_1d").to_blob(), 0)[0]
    assert central["reach"] == 2 and central["group"] == 1 and central["n_border"] == 1
    forward = iemlib.kkt_analyse_blob(C2.build_core("forward_1d").to_blob(), 0)[0]
    assert forward["reach"] == 1 and forward["S"] == 23 and forward["n_border"] == 1
    heat = C2.build_core("heat_central").to_blob()
    along_t = iemlib.kkt_analyse_blob(heat, 1)[0]
    assert along_t["reach"] == 1 and along_t["S"] == 7 and along_t["group"] == 1
    with pytest.raises(iemlib.IemError, match="a constraint row couples two lanes of the support grid"):
        iemlib.kkt_analyse_blob(heat, 0)
