"""The residual program on the MI355X: iem_lagrad and iem_eval_residual through model.ExaModel against the CPU oracle
(σ·om.grad(x) + om.jtprod(x, y), om.cons(x), om.obj(x)) to the 1e-10 relative of the parity suite, bitwise
against the separate calls, bit-reproducibility over repeated calls, kernel bookkeeping, θ updates, a graph capture and the
sharded refusal."""
import ctypes as C

import numpy as np
import pytest

import cases
import cases_param as CP
from pyoracle import OracleModel

pytestmark = pytest.mark.gpu
TOL = 1e-10
MODELS = CP.NAMES + CP.NO_PARAM
REPEAT = ("quadrotor_1000", "quadrotor_oc3_700", "shifted_pf_3000", "pandemic_20x3", "four_groups_param")


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


def witness(om, x, y, sigma):
    return sigma * om.grad(x) + (om.jtprod(x, y) if om.ncon else 0.0)


_models = {}


def model(name):
    """(core, blob, oracle): built once per model, shared by the tests"""
    if name not in _models:
        core = CP.build_core(name)
        blob = core.to_blob()
        _models[name] = (core, blob, OracleModel(blob))
    return _models[name]


@pytest.mark.parametrize("name", MODELS)
def test_values_and_bitwise_agreement(name, grid_mode):
    """NaN-poisoned outputs; lagrangian_grad and eval_residual against the oracle on both seeds; eval_residual's r, c and obj
    bitwise what lagrangian_grad, cons and obj_device write."""
    import torch
    from infiniteexamodels.jl_amd.model import ExaModel
    core, blob, om = model(name)
    gm = ExaModel(core, device=0, blob=blob)
    try:
        for seed in (0, 1):
            x, y = CP.eval_point(name, om, seed)
            sigma = 0.7 + 0.6 * seed
            xd, yd = torch.tensor(x, device="cuda"), torch.tensor(y, device="cuda")
            r1 = gm.lagrangian_grad(xd, yd, obj_weight=sigma, out=_poisoned(om.nvar))
            f, c, r = gm.eval_residual(xd, yd, obj_weight=sigma, c=_poisoned(om.ncon), out=_poisoned(om.nvar), obj=_poisoned(1))
            want = witness(om, x, y, sigma)
            errs = (rel(r1.cpu().numpy(), want), rel(r.cpu().numpy(), want), rel(c.cpu().numpy(), om.cons(x)),
                    abs(float(f.item()) - om.obj(x)) / max(1.0, abs(om.obj(x))))
            print(name, seed, grid_mode, " ".join(f"{e:.3e}" for e in errs), "max |want|", np.abs(want).max())
            assert np.abs(want).max() > 0 and np.isfinite(float(f.item()))
            assert max(errs) <= TOL
            assert torch.equal(_bits(r), _bits(r1))
            assert torch.equal(_bits(c), _bits(gm.cons(xd, _poisoned(om.ncon))))
            assert torch.equal(_bits(f), _bits(gm.obj_device(xd, _poisoned(1))))
        mine = gm.lagrangian_kernels()
        assert any(k["name"] == "iem_residual_all" and k["kind"] == "trial" for k in mine), [k["name"] for k in mine]
        assert not any(k["jit"] for k in gm.kernels() + mine), "the residual program was compiled at run time: build() must precompile it"
    finally:
        gm.close()


@pytest.mark.parametrize("name", REPEAT)
def test_repeated_calls_give_identical_bytes(name, built):
    import torch
    from infiniteexamodels.jl_amd.model import ExaModel
    core, blob, om = model(name)
    gm = ExaModel(core, device=0, blob=blob)
    try:
        x, y = CP.eval_point(name, om, 0)
        xd, yd = torch.tensor(x, device="cuda"), torch.tensor(y, device="cuda")
        r0 = gm.lagrangian_grad(xd, yd, obj_weight=0.7, out=_poisoned(om.nvar)).clone()
        f0, c0, q0 = (t.clone() for t in gm.eval_residual(xd, yd, obj_weight=0.7))
        assert rel(r0.cpu().numpy(), witness(om, x, y, 0.7)) <= TOL
        for _ in range(10):
            assert torch.equal(_bits(gm.lagrangian_grad(xd, yd, obj_weight=0.7, out=_poisoned(om.nvar))), _bits(r0))
            f, c, q = gm.eval_residual(xd, yd, obj_weight=0.7, c=_poisoned(om.ncon), out=_poisoned(om.nvar), obj=_poisoned(1))
            assert torch.equal(_bits(q), _bits(q0)) and torch.equal(_bits(c), _bits(c0)) and torch.equal(_bits(f), _bits(f0))
    finally:
        gm.close()


def _count(gm):
    from infiniteexamodels.jl_amd import lib as iemlib
    total = C.c_int32()
    iemlib.check(gm._L.iem_kernel_count(gm._h, C.byref(total)))
    return int(total.value)


@pytest.mark.parametrize("lag_first", [False, True])
def test_kernel_counts(lag_first, built):
    """lagrangian_prepare() returns the count of its program, lagrangian_kernels() is what iem_kernel_info lists last, and the
    other prepare calls report the same counts whether they are asked before or after."""
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.model import ExaModel
    core, blob, om = model("shifted_pf")
    gm = ExaModel(core, device=0, blob=blob)
    ref = ExaModel(core, device=0, blob=blob)      # never sees the residual program
    try:
        want = (ref.param_prepare(), ref.hppprod_prepare(), ref.param_coord_prepare())
        assert min(want) > 0
        own = gm.meta.n_kernels
        if lag_first:
            n = gm.lagrangian_prepare()
            assert _count(gm) == own + n
            got = (gm.param_prepare(), gm.hppprod_prepare(), gm.param_coord_prepare())
        else:
            got = (gm.param_prepare(), gm.hppprod_prepare(), gm.param_coord_prepare())
            before = _count(gm)
            n = gm.lagrangian_prepare()
            assert _count(gm) == before + n
            assert (gm.param_prepare(), gm.hppprod_prepare(), gm.param_coord_prepare()) == got
        assert got == want
        assert n == gm.lagrangian_prepare() == 4      # cons, obj, lagrad and the phase kernel; idempotent
        total = _count(gm)
        assert total == own + sum(want) + n
        mine = gm.lagrangian_kernels()
        assert [k["name"] for k in mine] == ["iem_cons_all", "iem_obj_all", "iem_lagrad_all", "iem_residual_all"]
        assert [k["kind"] for k in mine] == ["cons", "obj", "jtprod", "trial"]
        for j, k in enumerate(mine):      # ... the last ones of iem_kernel_info, and the next index is refused
            ki = iemlib.KernelInfo()
            iemlib.check(gm._L.iem_kernel_info(gm._h, total - n + j, C.byref(ki)))
            assert ki.name.decode() == k["name"] and int(ki.alg_bytes_read) == k["alg_bytes_read"] and int(ki.alg_bytes_written) == k["alg_bytes_written"]
        assert gm._L.iem_kernel_info(gm._h, total, C.byref(iemlib.KernelInfo())) == -4      # IEM_E_ARG
        by = {k["name"]: k for k in mine}
        assert by["iem_residual_all"]["alg_bytes_written"] == sum(by[n_]["alg_bytes_written"] for n_ in ("iem_cons_all", "iem_obj_all", "iem_lagrad_all"))
        assert by["iem_residual_all"]["alg_bytes_read"] < sum(by[n_]["alg_bytes_read"] for n_ in ("iem_cons_all", "iem_obj_all", "iem_lagrad_all"))
        # the θ programs' listings are still theirs
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
        x, y = CP.eval_point("shifted_pf", om, 0)
        xd, yd = torch.tensor(x, device="cuda"), torch.tensor(y, device="cuda")
        before = witness(om, x, y, 0.7)
        assert rel(gm.lagrangian_grad(xd, yd, obj_weight=0.7).cpu().numpy(), before) <= TOL
        th2 = np.asarray(core.theta) * 1.1 + 0.05
        om2 = OracleModel(blob)
        om2.set_parameter(0, th2)
        after = witness(om2, x, y, 0.7)
        assert rel(after, before) > 1e-6      # the check can tell, by the witness alone
        gm.set_parameter(0, th2)
        f, c, r = gm.eval_residual(xd, yd, obj_weight=0.7, c=_poisoned(om.ncon), out=_poisoned(om.nvar), obj=_poisoned(1))
        assert rel(gm.lagrangian_grad(xd, yd, obj_weight=0.7, out=_poisoned(om.nvar)).cpu().numpy(), after) <= TOL
        assert rel(r.cpu().numpy(), after) <= TOL and rel(c.cpu().numpy(), om2.cons(x)) <= TOL
        assert abs(float(f.item()) - om2.obj(x)) <= TOL * max(1.0, abs(om2.obj(x)))
    finally:
        gm.close()


def test_eval_residual_is_capturable(built):
    """lagrangian_prepare() does the synchronous set-up; one capture of eval_residual on quadrotor_1000, three replays, each
    bitwise equal to the direct call."""
    import torch
    from infiniteexamodels.jl_amd.model import ExaModel
    core, blob, om = model("quadrotor_1000")
    gm = ExaModel(core, device=0, blob=blob)
    try:
        x, y = CP.eval_point("quadrotor_1000", om, 0)
        xd, yd = torch.tensor(x, device="cuda"), torch.tensor(y, device="cuda")
        assert gm.lagrangian_prepare() > 0
        f0, c0, r0 = (t.clone() for t in gm.eval_residual(xd, yd, obj_weight=0.7, c=_poisoned(om.ncon), out=_poisoned(om.nvar), obj=_poisoned(1)))
        assert rel(r0.cpu().numpy(), witness(om, x, y, 0.7)) <= TOL
        f, c, r = _poisoned(1), _poisoned(om.ncon), _poisoned(om.nvar)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            gm.eval_residual(xd, yd, obj_weight=0.7, c=c, out=r, obj=f)
        for _ in range(3):
            for t in (f, c, r):
                t.fill_(float("nan"))
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(_bits(r), _bits(r0)) and torch.equal(_bits(c), _bits(c0)) and torch.equal(_bits(f), _bits(f0))
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
        f = torch.zeros(1, dtype=torch.float64, device="cuda")
        L = iemlib.lib()
        n = C.c_int32()
        for what, rc in (("iem_lagrad_prepare", L.iem_lagrad_prepare(sm._h, C.byref(n))),
                         ("iem_lagrad", L.iem_lagrad(sm._h, x.data_ptr(), y.data_ptr(), 1.0, x.data_ptr())),
                         ("iem_eval_residual", L.iem_eval_residual(sm._h, x.data_ptr(), y.data_ptr(), 1.0, y.data_ptr(), x.data_ptr(), f.data_ptr()))):
            assert rc == -4, (what, rc)      # IEM_E_ARG
        msg = L.iem_last_error().decode()
        assert "iem_eval_residual" in msg and "sharded" in msg and "all-reduce" in msg and "out of scope" in msg
        with pytest.raises(iemlib.IemError, match="sharded"):
            sm.lagrangian_grad(x, y)
        with pytest.raises(iemlib.IemError, match="sharded"):
            sm.eval_residual(x, y)
        with pytest.raises(iemlib.IemError, match="sharded"):
            sm.lagrangian_prepare()
    finally:
        sm.close()
