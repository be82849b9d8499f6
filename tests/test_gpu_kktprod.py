"""The KKT operator on the MI355X: iem_kktprod through model.ExaModel against the CPU oracle (om.hprod(x, y, u, σ) + om.jtprod(x, v)
to the 1e-10 relative of the parity suite), out_y bitwise iem_jprod, bit-reproducibility over repeated calls, kernel
bookkeeping, θ updates, a graph capture, the sharded refusal and the aliasing refusal."""
import ctypes as C

import numpy as np
import pytest

import cases
import cases_param as CP
import cases_scaled as CS
from pyoracle import OracleModel

pytestmark = pytest.mark.gpu
TOL = 1e-10
HAND = "nan_and_constant_rows"
MODELS = CP.NAMES + CP.NO_PARAM + [HAND]
REPEAT = ("quadrotor_1000", "quadrotor_oc3_700", "shifted_pf_3000", "pandemic_20x3", "four_groups_param", "farmer_5")
SIGMAS = (1.0, 0.0, -0.5)


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


def _bits(t):
    import torch
    return t.view(torch.int64)


def witness(om, x, y, u, v, sigma):
    return om.hprod(x, y, u, sigma) + (om.jtprod(x, v) if om.ncon else 0.0)


_models = {}


def model(name):
    """(core, blob, oracle): built once per model, shared by the tests"""
    if name not in _models:
        core = CS.nan_and_constant_rows() if name == HAND else CP.build_core(name)
        blob = core.to_blob()
        _models[name] = (core, blob, OracleModel(blob))
    return _models[name]


def point(name, om, seed=0):
    if name == HAND:
        x = np.asarray(om.x0, dtype=np.float64) + 0.05 * np.random.default_rng(seed).random(om.nvar)
        y = np.random.default_rng(seed + 1).standard_normal(om.ncon)
    else:
        x, y = CP.eval_point(name, om, seed)
    rng = np.random.default_rng(40 + seed)
    return x, y, rng.standard_normal(om.nvar), rng.standard_normal(om.ncon)


def dev(*arrays):
    import torch
    return tuple(torch.tensor(a, device="cuda") for a in arrays)


@pytest.mark.parametrize("name", MODELS)
def test_values_and_bitwise_agreement(name, grid_mode):
    """NaN-poisoned outputs, σ in {1, 0, -0.5}: out_x against the oracle, out_y bitwise iem_jprod; v = None is v = 0; the program
    was precompiled."""
    import torch
    from infiniteexamodels.jl_amd.model import ExaModel
    core, blob, om = model(name)
    gm = ExaModel(core, device=0, blob=blob)
    try:
        x, y, u, v = point(name, om)
        xd, yd, ud, vd = dev(x, y, u, v)
        jv = gm.jprod(xd, ud, _poisoned(om.ncon))
        for sigma in SIGMAS:
            ox, oy = gm.kktprod(xd, yd, ud, vd, obj_weight=sigma, out_x=_poisoned(om.nvar), out_y=_poisoned(om.ncon))
            want = witness(om, x, y, u, v, sigma)
            err = rel(ox.cpu().numpy(), want)
            print(name, sigma, grid_mode, f"{err:.3e}", "max |want|", np.abs(want).max())
            assert np.abs(want).max() > 0 and err <= TOL
            assert torch.equal(_bits(oy), _bits(jv))
        assert rel(jv.cpu().numpy(), om.jprod(x, u)) <= TOL
        hx, _ = gm.kktprod(xd, yd, ud, None, obj_weight=0.8, out_x=_poisoned(om.nvar), out_y=_poisoned(om.ncon))
        assert rel(hx.cpu().numpy(), om.hprod(x, y, u, 0.8)) <= TOL
        assert torch.equal(_bits(hx), _bits(gm.kktprod(xd, yd, ud, torch.zeros_like(vd), obj_weight=0.8)[0]))
        jx, jy = gm.kktprod(xd, yd, torch.zeros_like(ud), vd, obj_weight=0.8, out_x=_poisoned(om.nvar), out_y=_poisoned(om.ncon))
        assert rel(jx.cpu().numpy(), om.jtprod(x, v)) <= TOL and not jy.any()
        mine = gm.kkt_kernels()
        assert any(k["name"] == "iem_kktprod_all" and k["kind"] == "trial" for k in mine), [k["name"] for k in mine]
        assert not any(k["jit"] for k in gm.kernels() + mine), "the KKT operator was compiled at run time: build() must precompile it"
    finally:
        gm.close()


def test_no_constraints(built):
    """ncon == 0 through the C-ABI: NULL for y, v and out_y; an entry nothing touches is 0"""
    import torch
    from infiniteexamodels.jl_amd.model import ExaModel
    from test_kktprod import _unconstrained
    core = _unconstrained()
    blob = core.to_blob()
    om = OracleModel(blob)
    gm = ExaModel(core, device=0, blob=blob)
    try:
        rng = np.random.default_rng(0)
        x, u = om.x0 + 0.1 * rng.standard_normal(om.nvar), rng.standard_normal(om.nvar)
        xd, ud = dev(x, u)
        ox, oy = gm.kktprod(xd, None, ud, None, obj_weight=1.3, out_x=_poisoned(om.nvar))
        assert oy.numel() == 0 and rel(ox.cpu().numpy(), om.hprod(x, np.zeros(0), u, 1.3)) <= TOL
        assert not ox[-5:].any()
        assert [k["kind"] for k in gm.kkt_kernels()] == ["hprod"]
    finally:
        gm.close()


@pytest.mark.parametrize("name", REPEAT)
def test_repeated_calls_give_identical_bytes(name, built):
    import torch
    from infiniteexamodels.jl_amd.model import ExaModel
    core, blob, om = model(name)
    gm = ExaModel(core, device=0, blob=blob)
    try:
        x, y, u, v = point(name, om)
        xd, yd, ud, vd = dev(x, y, u, v)
        x0, y0 = (t.clone() for t in gm.kktprod(xd, yd, ud, vd, obj_weight=0.7, out_x=_poisoned(om.nvar), out_y=_poisoned(om.ncon)))
        assert rel(x0.cpu().numpy(), witness(om, x, y, u, v, 0.7)) <= TOL
        for _ in range(10):
            ox, oy = gm.kktprod(xd, yd, ud, vd, obj_weight=0.7, out_x=_poisoned(om.nvar), out_y=_poisoned(om.ncon))
            assert torch.equal(_bits(ox), _bits(x0)) and torch.equal(_bits(oy), _bits(y0))
    finally:
        gm.close()


def _count(gm):
    from infiniteexamodels.jl_amd import lib as iemlib
    total = C.c_int32()
    iemlib.check(gm._L.iem_kernel_count(gm._h, C.byref(total)))
    return int(total.value)


@pytest.mark.parametrize("kkt_first", [False, True])
def test_kernel_counts(kkt_first, built):
    """kkt_prepare() returns the count of its program, kkt_kernels() is what iem_kernel_info lists last, and the other prepare
    calls report the same counts — and the same listings — whether they are asked before or after."""
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.model import ExaModel
    core, blob, om = model("shifted_pf")
    gm = ExaModel(core, device=0, blob=blob)
    ref = ExaModel(core, device=0, blob=blob)      # never sees the KKT operator
    try:
        others = lambda m: (m.param_prepare(), m.hppprod_prepare(), m.param_coord_prepare(), m.lagrangian_prepare(), m.scaled_prepare())
        want = others(ref)
        assert min(want) > 0
        own = gm.meta.n_kernels
        if kkt_first:
            n = gm.kkt_prepare()
            assert _count(gm) == own + n
            got = others(gm)
        else:
            got = others(gm)
            before = _count(gm)
            n = gm.kkt_prepare()
            assert _count(gm) == before + n
            assert others(gm) == got
        assert got == want
        assert n == gm.kkt_prepare() == 3      # kkty, kktx and the one launch; idempotent
        total = _count(gm)
        assert total == own + sum(want) + n
        mine = gm.kkt_kernels()
        assert [k["name"] for k in mine] == ["iem_kkty_all", "iem_kktx_all", "iem_kktprod_all"]
        assert [k["kind"] for k in mine] == ["jprod", "hprod", "trial"]
        for j, k in enumerate(mine):      # ... the last ones of iem_kernel_info, and the next index is refused
            ki = iemlib.KernelInfo()
            iemlib.check(gm._L.iem_kernel_info(gm._h, total - n + j, C.byref(ki)))
            assert ki.name.decode() == k["name"] and int(ki.alg_bytes_read) == k["alg_bytes_read"] and int(ki.alg_bytes_written) == k["alg_bytes_written"]
        assert gm._L.iem_kernel_info(gm._h, total, C.byref(iemlib.KernelInfo())) == -4      # IEM_E_ARG
        by = {k["name"]: k for k in mine}
        assert by["iem_kktprod_all"]["alg_bytes_written"] == by["iem_kkty_all"]["alg_bytes_written"] + by["iem_kktx_all"]["alg_bytes_written"]
        assert by["iem_kktprod_all"]["alg_bytes_read"] < by["iem_kkty_all"]["alg_bytes_read"] + by["iem_kktx_all"]["alg_bytes_read"]
        # the other programs' listings are still theirs
        assert all(k["name"].startswith(("iem_rowmax", "iem_cons_scaled", "iem_jac_scaled")) for k in gm.scaled_kernels()) and len(gm.scaled_kernels()) == want[4]
        assert [k["name"] for k in gm.lagrangian_kernels()] == ["iem_cons_all", "iem_obj_all", "iem_lagrad_all", "iem_residual_all"]
        assert all(k["name"].startswith(("iem_jacp", "iem_hessp")) for k in gm.param_coord_kernels())
        assert all(k["name"].startswith("iem_hppprod") for k in gm.hppprod_kernels())
    finally:
        gm.close(); ref.close()


def test_the_result_follows_the_current_theta(built):
    import torch
    from infiniteexamodels.jl_amd.model import ExaModel
    core, blob, om = model("shifted_pf")
    gm = ExaModel(core, device=0, blob=blob)
    try:
        x, y, u, v = point("shifted_pf", om)
        xd, yd, ud, vd = dev(x, y, u, v)
        before = witness(om, x, y, u, v, 0.7)
        assert rel(gm.kktprod(xd, yd, ud, vd, obj_weight=0.7)[0].cpu().numpy(), before) <= TOL
        th2 = np.asarray(core.theta) * 1.1 + 0.05
        om2 = OracleModel(blob)
        om2.set_parameter(0, th2)
        after = witness(om2, x, y, u, v, 0.7)
        assert rel(after, before) > 1e-6      # the check can tell, by the witness alone
        gm.set_parameter(0, th2)
        ox, oy = gm.kktprod(xd, yd, ud, vd, obj_weight=0.7, out_x=_poisoned(om.nvar), out_y=_poisoned(om.ncon))
        assert rel(ox.cpu().numpy(), after) <= TOL and rel(oy.cpu().numpy(), om2.jprod(x, u)) <= TOL
    finally:
        gm.close()


def test_kktprod_is_capturable(built):
    """kkt_prepare() does the synchronous set-up; one capture of kktprod on quadrotor_1000, three replays, each bitwise equal to
    the direct call."""
    import torch
    from infiniteexamodels.jl_amd.model import ExaModel
    core, blob, om = model("quadrotor_1000")
    gm = ExaModel(core, device=0, blob=blob)
    try:
        x, y, u, v = point("quadrotor_1000", om)
        xd, yd, ud, vd = dev(x, y, u, v)
        assert gm.kkt_prepare() > 0
        x0, y0 = (t.clone() for t in gm.kktprod(xd, yd, ud, vd, obj_weight=0.7, out_x=_poisoned(om.nvar), out_y=_poisoned(om.ncon)))
        assert rel(x0.cpu().numpy(), witness(om, x, y, u, v, 0.7)) <= TOL
        ox, oy = _poisoned(om.nvar), _poisoned(om.ncon)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            gm.kktprod(xd, yd, ud, vd, obj_weight=0.7, out_x=ox, out_y=oy)
        for _ in range(3):
            ox.fill_(float("nan")); oy.fill_(float("nan"))
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(_bits(ox), _bits(x0)) and torch.equal(_bits(oy), _bits(y0))
    finally:
        gm.close()


def test_sharded_handle_refuses(built):
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.model import ExaModel
    sm = ExaModel.sharded(cases.build_core("quadrotor_100").to_blob(), 1, 0, 2, device=0)
    try:
        x = torch.zeros(sm.meta.nvar, dtype=torch.float64, device="cuda")
        y = torch.zeros(sm.meta.ncon, dtype=torch.float64, device="cuda")
        ox, oy = torch.zeros_like(x), torch.zeros_like(y)
        L = iemlib.lib()
        n = C.c_int32()
        for what, rc in (("iem_kktprod_prepare", L.iem_kktprod_prepare(sm._h, C.byref(n))),
                         ("iem_kktprod", L.iem_kktprod(sm._h, x.data_ptr(), y.data_ptr(), 1.0, x.data_ptr(), y.data_ptr(), ox.data_ptr(), oy.data_ptr()))):
            assert rc == -4, (what, rc)      # IEM_E_ARG
        msg = L.iem_last_error().decode()
        assert "iem_kktprod" in msg and "sharded" in msg and "out of scope" in msg
        with pytest.raises(iemlib.IemError, match="sharded"):
            sm.kktprod(x, y, x)
        with pytest.raises(iemlib.IemError, match="sharded"):
            sm.kkt_prepare()
    finally:
        sm.close()


def test_aliasing_is_refused(built):
    """an output that overlaps an input (or the other output) is IEM_E_ARG, and nothing is written"""
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.model import ExaModel
    core, blob, om = model("quadrotor_5")
    gm = ExaModel(core, device=0, blob=blob)
    try:
        x, y, u, v = point("quadrotor_5", om)
        xd, yd, ud, vd = dev(x, y, u, v)
        ox, oy = _poisoned(om.nvar), _poisoned(om.ncon)
        both = _poisoned(om.nvar + om.ncon)
        L, p = gm._L, lambda t: t.data_ptr()
        call = lambda u_, v_, a, b: L.iem_kktprod(gm._h, p(xd), p(yd), 1.0, u_, v_, a, b)
        assert call(p(ud), p(vd), p(ox), p(oy)) == 0
        for what, rc in (("out_x is u", call(p(ud), p(vd), p(ud), p(oy))), ("out_x is x", call(p(ud), p(vd), p(xd), p(oy))),
                         ("out_y is v", call(p(ud), p(vd), p(ox), p(vd))), ("out_y is y", call(p(ud), p(vd), p(ox), p(yd))),
                         ("out_x inside u", call(p(both), p(vd), p(both) + 8 * 4, p(oy))),
                         ("out_y inside out_x", call(p(ud), p(vd), p(both), p(both) + 8 * (om.nvar - 1)))):
            assert rc == -4, (what, rc)
            assert "overlap" in L.iem_last_error().decode()
        torch.cuda.synchronize()
        assert torch.equal(xd.cpu(), torch.tensor(x)) and torch.equal(ud.cpu(), torch.tensor(u)) and torch.isnan(both).all()
        # side by side in one array is fine: [out_x | out_y]
        assert call(p(ud), p(vd), p(both), p(both) + 8 * om.nvar) == 0
        torch.cuda.synchronize()
        assert torch.equal(_bits(both[:om.nvar]), _bits(ox)) and torch.equal(_bits(both[om.nvar:]), _bits(oy))
    finally:
        gm.close()
