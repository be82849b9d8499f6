"""The scaled program on the MI355X: iem_jac_rowmax, iem_cons_scaled and iem_jac_coord_scaled through model.ExaModel against
the CPU oracle to the 1e-10 relative of the parity suite, the three bitwise identities against jac_coord / cons
on the same handle, bit-reproducibility, kernel bookkeeping, θ updates, a graph capture, NaN rows, the sharded refusal, and
scaling.gradient_scaling / ScaledModel against contrib.ipm._Scaled."""
import ctypes as C

import numpy as np
import pytest

import cases
import cases_param as CP
import cases_scaled as CS
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


def factors(n, seed):
    """s in [2^-3, 2^3], no entry a power of two"""
    s = np.exp2(np.random.default_rng(100 + seed).uniform(-3.0, 3.0, n))
    assert ((s >= 0.125) & (s <= 8.0)).all() and (np.frexp(s)[0] != 0.5).all()
    return s


def _amax(rows, vals, m):
    import torch
    return torch.zeros(m, dtype=torch.float64, device="cuda").scatter_reduce(0, rows, vals.abs(), reduce="amax")


_models = {}


def model(name):
    """(core, blob, oracle, rows of the oracle's jac_structure): built once per model, shared by the tests"""
    if name not in _models:
        core = CS.nan_and_constant_rows() if name == "nan_and_constant_rows" else CP.build_core(name)
        blob = core.to_blob()
        om = OracleModel(blob)
        _models[name] = (core, blob, om, om.jac_structure(base=0)[0])
    return _models[name]


@pytest.mark.parametrize("name", MODELS)
def test_values_and_the_bitwise_contract(name, grid_mode):
    """NaN-poisoned outputs, both seeds: the three calls against the oracle, and bitwise fl(s[row]·v) / fl(s·c) / the per-row
    maximum of |v| of what jac_coord and cons write on the same handle."""
    import torch
    from infiniteexamodels.jl_amd.model import ExaModel
    core, blob, om, rows = model(name)
    gm = ExaModel(core, device=0, blob=blob)
    try:
        rd = torch.tensor(rows, device="cuda")
        if om.ncon == 0:      # nothing to launch, no kernel, no error
            xd, e = torch.tensor(np.asarray(om.x0, dtype=np.float64), device="cuda"), _poisoned(0)
            assert gm.jac_row_maxabs(xd).numel() == gm.cons_scaled(xd, e).numel() == gm.jac_coord_scaled(xd, e).numel() == 0
            assert gm.scaled_kernels() == []
            return
        for seed in (0, 1):
            x, _ = CP.eval_point(name, om, seed)
            s = factors(om.ncon, seed)
            xd, sd = torch.tensor(x, device="cuda"), torch.tensor(s, device="cuda")
            rm = gm.jac_row_maxabs(xd, _poisoned(om.ncon))
            cs = gm.cons_scaled(xd, sd, _poisoned(om.ncon))
            js = gm.jac_coord_scaled(xd, sd, _poisoned(om.nnzj))
            jo, co = om.jac_coord(x), om.cons(x)
            want_rm = np.zeros(om.ncon)
            np.maximum.at(want_rm, rows, np.abs(jo))
            errs = (rel(rm.cpu().numpy(), want_rm), rel(cs.cpu().numpy(), s * co), rel(js.cpu().numpy(), s[rows] * jo))
            print(name, seed, grid_mode, " ".join(f"{e:.3e}" for e in errs), "max rowmax", want_rm.max())
            assert want_rm.max() > 0 and max(errs) <= TOL
            j, c = gm.jac_coord(xd, _poisoned(om.nnzj)), gm.cons(xd, _poisoned(om.ncon))
            assert torch.equal(_bits(js), _bits(sd[rd] * j))
            assert torch.equal(_bits(cs), _bits(sd * c))
            assert torch.equal(_bits(rm), _bits(_amax(rd, j, om.ncon)))
        mine = gm.scaled_kernels()
        assert {k["kind"] for k in mine} == {"jprod", "cons", "jac"}
        assert all(k["name"].startswith(("iem_rowmax", "iem_cons_scaled", "iem_jac_scaled")) for k in mine), [k["name"] for k in mine]
        assert not any(k["jit"] for k in gm.kernels() + mine), "the scaled program was compiled at run time: build() must precompile it"
    finally:
        gm.close()


@pytest.mark.parametrize("name", REPEAT)
def test_repeated_calls_give_identical_bytes(name, built):
    import torch
    from infiniteexamodels.jl_amd.model import ExaModel
    core, blob, om, rows = model(name)
    gm = ExaModel(core, device=0, blob=blob)
    try:
        x, _ = CP.eval_point(name, om, 0)
        xd, sd = torch.tensor(x, device="cuda"), torch.tensor(factors(om.ncon, 0), device="cuda")
        first = [gm.jac_row_maxabs(xd).clone(), gm.cons_scaled(xd, sd).clone(), gm.jac_coord_scaled(xd, sd).clone()]
        for _ in range(10):
            again = (gm.jac_row_maxabs(xd, _poisoned(om.ncon)), gm.cons_scaled(xd, sd, _poisoned(om.ncon)), gm.jac_coord_scaled(xd, sd, _poisoned(om.nnzj)))
            assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(again, first))
    finally:
        gm.close()


def _count(gm):
    from infiniteexamodels.jl_amd import lib as iemlib
    total = C.c_int32()
    iemlib.check(gm._L.iem_kernel_count(gm._h, C.byref(total)))
    return int(total.value)


@pytest.mark.parametrize("scaled_first", [False, True])
def test_kernel_counts(scaled_first, built):
    """scaled_prepare() returns the count of its program, scaled_kernels() is what iem_kernel_info lists last, every other
    prepare call reports the same count whether it is asked before or after, and the other programs' listings stay theirs."""
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.model import ExaModel
    core, blob, om, _ = model("shifted_pf")
    gm = ExaModel(core, device=0, blob=blob)
    ref = ExaModel(core, device=0, blob=blob)      # never sees the scaled program
    try:
        others = lambda m: (m.param_prepare(), m.hppprod_prepare(), m.param_coord_prepare(), m.lagrangian_prepare())
        want = others(ref)
        assert min(want) > 0
        own = gm.meta.n_kernels
        if scaled_first:
            n = gm.scaled_prepare()
            assert _count(gm) == own + n
            got = others(gm)
        else:
            got = others(gm)
            before = _count(gm)
            n = gm.scaled_prepare()
            assert _count(gm) == before + n
            assert others(gm) == got
        assert got == want
        assert n == gm.scaled_prepare() == 3      # cons_scaled, jac_scaled, rowmax; idempotent
        total = _count(gm)
        assert total == own + sum(want) + n
        mine = gm.scaled_kernels()
        assert sorted(k["kind"] for k in mine) == ["cons", "jac", "jprod"]
        assert all(k["name"].startswith(p) for k, p in zip(sorted(mine, key=lambda k: k["kind"]), ("iem_cons_scaled", "iem_jac_scaled", "iem_rowmax")))
        for j, k in enumerate(mine):      # ... the last ones of iem_kernel_info, and the next index is refused
            ki = iemlib.KernelInfo()
            iemlib.check(gm._L.iem_kernel_info(gm._h, total - n + j, C.byref(ki)))
            assert ki.name.decode() == k["name"] and int(ki.alg_bytes_read) == k["alg_bytes_read"] and int(ki.alg_bytes_written) == k["alg_bytes_written"]
        assert gm._L.iem_kernel_info(gm._h, total, C.byref(iemlib.KernelInfo())) == -4      # IEM_E_ARG
        by = {k["kind"]: k for k in mine}
        assert by["jprod"]["alg_bytes_written"] == 8 * om.ncon == by["cons"]["alg_bytes_written"] and by["jac"]["alg_bytes_written"] == 8 * om.nnzj
        # the other programs' listings are still theirs
        assert [k["name"] for k in gm.lagrangian_kernels()] == [k["name"] for k in ref.lagrangian_kernels()] == ["iem_cons_all", "iem_obj_all", "iem_lagrad_all", "iem_residual_all"]
        assert gm.param_coord_kernels() == ref.param_coord_kernels()
        assert all(k["name"].startswith(("iem_jacp", "iem_hessp")) for k in gm.param_coord_kernels())
    finally:
        gm.close(); ref.close()


def test_the_result_follows_the_current_theta(built):
    import torch
    from infiniteexamodels.jl_amd.model import ExaModel
    core, blob, om, rows = model("shifted_pf")
    gm = ExaModel(core, device=0, blob=blob)
    try:
        x, _ = CP.eval_point("shifted_pf", om, 0)
        s = factors(om.ncon, 0)
        xd, sd = torch.tensor(x, device="cuda"), torch.tensor(s, device="cuda")

        def wit(o):
            rm = np.zeros(o.ncon)
            np.maximum.at(rm, rows, np.abs(o.jac_coord(x)))
            return rm, s * o.cons(x), s[rows] * o.jac_coord(x)

        def got():
            return (gm.jac_row_maxabs(xd, _poisoned(om.ncon)).cpu().numpy(), gm.cons_scaled(xd, sd, _poisoned(om.ncon)).cpu().numpy(),
                    gm.jac_coord_scaled(xd, sd, _poisoned(om.nnzj)).cpu().numpy())
        before = wit(om)
        assert max(rel(a, b) for a, b in zip(got(), before)) <= TOL
        th2 = np.asarray(core.theta) * 1.1 + 0.05
        om2 = OracleModel(blob)
        om2.set_parameter(0, th2)
        after = wit(om2)
        assert min(rel(a, b) for a, b in zip(after, before)) > 1e-6      # the check can tell, by the witness alone
        gm.set_parameter(0, th2)
        assert max(rel(a, b) for a, b in zip(got(), after)) <= TOL
    finally:
        gm.close()


def test_scaled_calls_are_capturable(built):
    """scaled_prepare() does the synchronous set-up; one capture of jac_coord_scaled + cons_scaled on quadrotor_1000, three
    replays, each bitwise the direct call."""
    import torch
    from infiniteexamodels.jl_amd.model import ExaModel
    core, blob, om, rows = model("quadrotor_1000")
    gm = ExaModel(core, device=0, blob=blob)
    try:
        x, _ = CP.eval_point("quadrotor_1000", om, 0)
        s = factors(om.ncon, 0)
        xd, sd = torch.tensor(x, device="cuda"), torch.tensor(s, device="cuda")
        assert gm.scaled_prepare() > 0
        j0 = gm.jac_coord_scaled(xd, sd, _poisoned(om.nnzj)).clone()
        c0 = gm.cons_scaled(xd, sd, _poisoned(om.ncon)).clone()
        assert rel(j0.cpu().numpy(), s[rows] * om.jac_coord(x)) <= TOL and rel(c0.cpu().numpy(), s * om.cons(x)) <= TOL
        j, c = _poisoned(om.nnzj), _poisoned(om.ncon)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            gm.jac_coord_scaled(xd, sd, j)
            gm.cons_scaled(xd, sd, c)
        for _ in range(3):
            j.fill_(float("nan")); c.fill_(float("nan"))
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(_bits(j), _bits(j0)) and torch.equal(_bits(c), _bits(c0))
    finally:
        gm.close()


def test_nan_row_and_rows_without_a_slot(grid_mode):
    """The hand-built rows of the CPU file: the NaN entry of a row (second slot in one row, first in another) makes that row
    NaN in all three outputs and nothing else; a row of item data alone has the maximum 0.0 with the sign bit clear."""
    import torch
    from infiniteexamodels.jl_amd.model import ExaModel
    core, blob, om, rows = model("nan_and_constant_rows")
    gm = ExaModel(core, device=0, blob=blob)
    try:
        x = CS.nan_point(om)
        s = factors(om.ncon, 0)
        nan_rows, no_slot = CS.rows_of()
        xd, sd = torch.tensor(x, device="cuda"), torch.tensor(s, device="cuda")
        rm = gm.jac_row_maxabs(xd, _poisoned(om.ncon)).cpu().numpy()
        cs = gm.cons_scaled(xd, sd, _poisoned(om.ncon)).cpu().numpy()
        js = gm.jac_coord_scaled(xd, sd, _poisoned(om.nnzj)).cpu().numpy()
        for out in (rm, cs):
            assert np.array_equal(np.flatnonzero(np.isnan(out)), nan_rows) and np.isfinite(np.delete(out, nan_rows)).all()
        assert np.array_equal(np.unique(rows[np.isnan(js)]), nan_rows) and np.isnan(js).sum() == 2
        assert np.isfinite(js[~np.isnan(js)]).all()
        assert not rm[no_slot].any() and not np.signbit(rm[no_slot]).any()
        assert not any(k["jit"] for k in gm.kernels() + gm.scaled_kernels())
    finally:
        gm.close()


def test_sharded_handle_refuses(built):
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.model import ExaModel
    sm = ExaModel.sharded(cases.build_core("quadrotor_100").to_blob(), 1, 0, 2, device=0)
    try:
        x = torch.zeros(sm.meta.nvar, dtype=torch.float64, device="cuda")
        s = torch.ones(sm.meta.ncon, dtype=torch.float64, device="cuda")
        c = torch.zeros(sm.meta.ncon, dtype=torch.float64, device="cuda")
        v = torch.zeros(sm.meta.nnzj, dtype=torch.float64, device="cuda")
        L = iemlib.lib()
        n = C.c_int32()
        for what, call in (("iem_scaled_prepare", lambda: L.iem_scaled_prepare(sm._h, C.byref(n))),
                           ("iem_jac_rowmax", lambda: L.iem_jac_rowmax(sm._h, x.data_ptr(), c.data_ptr())),
                           ("iem_cons_scaled", lambda: L.iem_cons_scaled(sm._h, x.data_ptr(), s.data_ptr(), c.data_ptr())),
                           ("iem_jac_coord_scaled", lambda: L.iem_jac_coord_scaled(sm._h, x.data_ptr(), s.data_ptr(), v.data_ptr()))):
            assert call() == -4, what      # IEM_E_ARG
            msg = L.iem_last_error().decode()
            assert what in msg and "sharded" in msg and "out of scope" in msg, msg
        for call in (lambda: sm.scaled_prepare(), lambda: sm.jac_row_maxabs(x), lambda: sm.cons_scaled(x, s), lambda: sm.jac_coord_scaled(x, s)):
            with pytest.raises(iemlib.IemError, match="sharded"):
                call()
    finally:
        sm.close()


@pytest.mark.parametrize("name", ["nan_and_constant_rows", "quadrotor_1000"])
def test_scaling_module_against_the_solver_side_scaling(name, built):
    """scaling.gradient_scaling gives bitwise the df / dc of contrib.ipm._Scaled(gm, x0, 100.0); ScaledModel's cons, jac_coord,
    hess_coord and grad are bitwise what _Scaled returns at a second point."""
    import torch
    from infiniteexamodels.jl_amd import scaling
    from infiniteexamodels.jl_amd.contrib.ipm import _Scaled
    from infiniteexamodels.jl_amd.model import ExaModel
    core, blob, om, rows = model(name)
    gm = ExaModel(core, device=0, blob=blob)
    try:
        x0 = torch.tensor(np.asarray(om.x0, dtype=np.float64), device="cuda")
        old = _Scaled(gm, x0, 100.0)
        df, dc = scaling.gradient_scaling(gm, x0)
        assert df == old.df and torch.equal(_bits(dc), _bits(old.dc))
        if name == "nan_and_constant_rows":
            assert bool((dc != 1.0).any()) and bool((dc == 1.0).any())      # the difference rows (1/h = 699) are scaled, the others not
        sm = scaling.ScaledModel(gm, df, dc)
        x = x0 + 0.05 * torch.tensor(np.random.default_rng(3).random(om.nvar), device="cuda")
        y = torch.tensor(np.random.default_rng(4).standard_normal(om.ncon), device="cuda")
        jac, hess = _poisoned(om.nnzj), _poisoned(om.nnzh)
        old.jac_hess_coord(x, y, jac, hess, obj_weight=0.7)
        assert torch.equal(_bits(sm.cons(x, _poisoned(om.ncon))), _bits(old.cons(x)))
        assert torch.equal(_bits(sm.jac_coord(x, _poisoned(om.nnzj))), _bits(jac))
        assert torch.equal(_bits(sm.hess_coord(x, y, _poisoned(om.nnzh), obj_weight=0.7)), _bits(hess))
        assert torch.equal(_bits(sm.grad(x)), _bits(old.grad(x)))
        assert np.array_equal(sm.meta.lcon, old.meta.lcon) and np.array_equal(sm.meta.ucon, old.meta.ucon)
    finally:
        gm.close()
