"""The scaled solver phases on the MI355X: iem_eval_trial_scaled, iem_eval_accepted_scaled, iem_grad_scaled and
iem_hess_coord_scaled through model.ExaModel against the CPU oracle to the 1e-10 relative of the parity suite
and against the calls of the same handle they are defined by — c, jac, hess and f bitwise, the gradient as IEEE values for
the factors 1 and 2^k — then bit-reproducibility, kernel bookkeeping, θ updates, graph captures, the deferred objective, the
member-launch fallback, the sharded refusal, and scaling.ScaledModel against contrib.ipm._Scaled."""
import ctypes as C

import numpy as np
import pytest

import cases
import cases_param as CP
import cases_scaled as CS
import cases_scaled_phases as CD
from pyoracle import OracleModel
from test_gpu_scaled import REPEAT

pytestmark = pytest.mark.gpu
TOL = 1e-10
HAND = "nan_and_constant_rows"
MODELS = CP.NAMES + CP.NO_PARAM + [HAND] + list(CD.DEGENERATE)
SP_NAMES = ("iem_sp_cons", "iem_sp_jac", "iem_sp_hess", "iem_sp_obj", "iem_sp_grad", "iem_sp_trial_all", "iem_sp_accepted_all")


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


def _fbits(v):
    return np.float64(v).view(np.int64)


def same_values(a, b):
    """equal as IEEE values, NaNs in the same places; the sign of a zero is not compared"""
    a, b = a.cpu().numpy(), b.cpu().numpy()
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and bool((a[~na] == b[~nb]).all())


def factors(n, which, seed=0):
    return np.random.default_rng(200 + seed).uniform(0.1, 2.0, n) if which == "random" else np.ones(n)


_models = {}


def model(name):
    """(core, blob, oracle, rows of the oracle's jac_structure): built once per model, shared by the tests"""
    if name not in _models:
        core = CS.nan_and_constant_rows() if name == HAND else CD.DEGENERATE[name]() if name in CD.DEGENERATE else CP.build_core(name)
        blob = core.to_blob()
        om = OracleModel(blob)
        _models[name] = (core, blob, om, om.jac_structure(base=0)[0])
    return _models[name]


def point(name, om, seed=0):
    if name == HAND or name in CD.DEGENERATE:
        x = np.asarray(om.x0, dtype=np.float64) + 0.05 * np.random.default_rng(seed).random(om.nvar)
    else:
        x, _ = CP.eval_point(name, om, seed)
    return x, np.random.default_rng(seed + 1).standard_normal(om.ncon)


def _dev(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")


@pytest.mark.parametrize("name", MODELS)
def test_contracts_through_the_c_abi(name, grid_mode):
    """NaN-poisoned outputs, both code shapes, s random and s = 1: values against the oracle, contracts 1 - 4 against the calls of
    the same handle, the phases bitwise their members."""
    import torch
    from infiniteexamodels.jl_amd.model import ExaModel
    core, blob, om, rows = model(name)
    gm = ExaModel(core, device=0, blob=blob)
    try:
        rd = torch.tensor(rows, device="cuda")
        x, y = point(name, om)
        xd, yd = _dev(x), _dev(y)
        sf, sigma = 0.3, 0.7
        w = sigma * sf
        g0 = gm.grad(xd, _poisoned(om.nvar))
        f0 = gm.obj(xd)
        for which in ("random", "ones"):
            s = factors(om.ncon, which)
            sd = _dev(s)
            f, c = gm.eval_trial_scaled(xd, sd, sf, _poisoned(om.ncon))
            g, jac, hess = gm.eval_accepted_scaled(xd, yd, sd, sf, _poisoned(om.nvar), _poisoned(om.nnzj), _poisoned(om.nnzh), obj_weight=sigma)
            errs = (rel(c.cpu().numpy(), s * om.cons(x)), rel(jac.cpu().numpy(), s[rows] * om.jac_coord(x)),
                    rel(hess.cpu().numpy(), om.hess_coord(x, y * s, w)), rel(g.cpu().numpy(), sf * om.grad(x)),
                    abs(f - sf * om.obj(x)) / max(1.0, abs(om.obj(x))))
            print(name, which, grid_mode, " ".join(f"{e:.3e}" for e in errs))
            assert max(errs) <= TOL
            # 1: constraints and Jacobian
            assert torch.equal(_bits(c), _bits(gm.cons_scaled(xd, sd, _poisoned(om.ncon))))
            assert torch.equal(_bits(jac), _bits(gm.jac_coord_scaled(xd, sd, _poisoned(om.nnzj))))
            # 2: the Hessian: iem_hess_coord with y∘s formed by one float64 multiply per row
            hs = gm.hess_coord_scaled(xd, yd, sd, _poisoned(om.nnzh), obj_weight=w)
            assert torch.equal(_bits(hs), _bits(gm.hess_coord(xd, yd * sd, _poisoned(om.nnzh), obj_weight=w)))
            assert torch.equal(_bits(hess), _bits(hs))
            # 3: the objective
            assert _fbits(f) == _fbits(sf * f0)
            # 4: the gradient of the phase is the gradient call's
            assert torch.equal(_bits(g), _bits(gm.grad_scaled(xd, sf, _poisoned(om.nvar))))
        assert same_values(gm.grad_scaled(xd, 1.0, _poisoned(om.nvar)), g0)
        for k in (-1, -10):
            assert same_values(gm.grad_scaled(xd, 2.0 ** k, _poisoned(om.nvar)), g0 * 2.0 ** k)
        mine = gm.scaled_phase_kernels()
        assert mine and all(k["name"].startswith(SP_NAMES) for k in mine), [k["name"] for k in mine]
        if om.ncon and name != "no_objective":
            assert {"iem_sp_trial_all", "iem_sp_accepted_all"} <= {k["name"] for k in mine}
        assert not any(k["jit"] for k in gm.kernels() + mine), "the program was compiled at run time: build() must precompile it"
    finally:
        gm.close()


@pytest.mark.parametrize("name", REPEAT)
def test_repeated_calls_give_identical_bytes(name, built):
    import torch
    from infiniteexamodels.jl_amd.model import ExaModel
    core, blob, om, rows = model(name)
    gm = ExaModel(core, device=0, blob=blob)
    try:
        x, y = point(name, om)
        xd, yd, sd = _dev(x), _dev(y), _dev(factors(om.ncon, "random"))
        f0, c0 = gm.eval_trial_scaled(xd, sd, 0.3)
        first = [t.clone() for t in gm.eval_accepted_scaled(xd, yd, sd, 0.3, obj_weight=0.7)] + [c0.clone()]
        for _ in range(10):
            f, c = gm.eval_trial_scaled(xd, sd, 0.3, _poisoned(om.ncon))
            again = list(gm.eval_accepted_scaled(xd, yd, sd, 0.3, _poisoned(om.nvar), _poisoned(om.nnzj), _poisoned(om.nnzh), obj_weight=0.7)) + [c]
            assert _fbits(f) == _fbits(f0) and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(again, first))
    finally:
        gm.close()


def _count(gm):
    from infiniteexamodels.jl_amd import lib as iemlib
    total = C.c_int32()
    iemlib.check(gm._L.iem_kernel_count(gm._h, C.byref(total)))
    return int(total.value)


@pytest.mark.parametrize("phases_first", [False, True])
def test_kernel_counts(phases_first, built):
    """scaled_phase_prepare() returns the count of its program, scaled_phase_kernels() is what iem_kernel_info lists LAST —
    behind the KKT operator's — whether it is prepared before or after the others; every other prepare call and listing stays."""
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.model import ExaModel
    core, blob, om, _ = model("shifted_pf")
    gm = ExaModel(core, device=0, blob=blob)
    ref = ExaModel(core, device=0, blob=blob)      # never sees this program
    try:
        others = lambda m: (m.param_prepare(), m.hppprod_prepare(), m.param_coord_prepare(), m.lagrangian_prepare(), m.scaled_prepare(), m.kkt_prepare())
        want = others(ref)
        assert min(want) > 0
        own = gm.meta.n_kernels
        if phases_first:
            n = gm.scaled_phase_prepare()
            assert _count(gm) == own + n
            got = others(gm)
        else:
            got = others(gm)
            before = _count(gm)
            n = gm.scaled_phase_prepare()
            assert _count(gm) == before + n
            assert others(gm) == got
        assert got == want and gm.meta.n_kernels == own
        assert n == gm.scaled_phase_prepare() == 7      # five kinds and two phases; idempotent
        total = _count(gm)
        assert total == own + sum(want) + n
        mine = gm.scaled_phase_kernels()
        assert [k["kind"] for k in mine] == ["cons", "jac", "hess", "obj", "grad", "trial", "accepted"]
        assert [k["name"] for k in mine] == [f"iem_sp_{k}_all" for k in ("cons", "jac", "hess", "obj", "grad", "trial", "accepted")]
        for j, k in enumerate(mine):      # ... the last ones of iem_kernel_info, and the next index is refused
            ki = iemlib.KernelInfo()
            iemlib.check(gm._L.iem_kernel_info(gm._h, total - n + j, C.byref(ki)))
            assert ki.name.decode() == k["name"] and int(ki.alg_bytes_read) == k["alg_bytes_read"] and int(ki.alg_bytes_written) == k["alg_bytes_written"]
        assert gm._L.iem_kernel_info(gm._h, total, C.byref(iemlib.KernelInfo())) == -4      # IEM_E_ARG
        by = {k["kind"]: k for k in mine}
        assert by["trial"]["alg_bytes_written"] == 8 * (om.ncon + 1) and by["accepted"]["alg_bytes_written"] >= 8 * (om.nnzj + om.nnzh + om.nvar)
        # the other programs' listings are still theirs
        assert gm.kkt_kernels() == ref.kkt_kernels() and all(k["name"].startswith("iem_kkt") for k in gm.kkt_kernels())
        assert gm.scaled_kernels() == ref.scaled_kernels() and len(gm.scaled_kernels()) == 3
        assert gm.lagrangian_kernels() == ref.lagrangian_kernels() and gm.param_coord_kernels() == ref.param_coord_kernels()
    finally:
        gm.close(); ref.close()


def test_kernel_order_does_not_depend_on_the_order_of_set_up(built):
    """All seven prepare calls in reverse order on one handle, in forward order on another: iem_kernel_count, every
    iem_kernel_info entry and every *_kernels() listing agree — the public order is the library's table of programs,
    not the order in which a caller happened to set them up."""
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.model import ExaModel
    core, blob, _, _ = model("shifted_pf")
    prepares = ("param_prepare", "hppprod_prepare", "param_coord_prepare", "lagrangian_prepare", "scaled_prepare", "kkt_prepare", "scaled_phase_prepare")
    listings = ("param_kernels", "hppprod_kernels", "param_coord_kernels", "lagrangian_kernels", "scaled_kernels", "kkt_kernels", "scaled_phase_kernels")
    fwd = ExaModel(core, device=0, blob=blob)
    rev = ExaModel(core, device=0, blob=blob)
    try:
        counts = {p: getattr(rev, p)() for p in reversed(prepares)}
        assert counts == {p: getattr(fwd, p)() for p in prepares} and min(counts.values()) > 0
        total = _count(fwd)
        assert total == _count(rev) == fwd.meta.n_kernels + sum(counts.values())

        def info(gm, k):
            ki = iemlib.KernelInfo()
            iemlib.check(gm._L.iem_kernel_info(gm._h, k, C.byref(ki)))
            return ki.name.decode(), int(ki.kind), tuple(ki.grid)
        for k in range(total):
            assert info(fwd, k) == info(rev, k), k
        first = fwd.meta.n_kernels      # ... and it is the order of the prepare calls above: each program's kernels behind the previous one's
        for p, l in zip(prepares, listings):
            mine = getattr(fwd, l)()
            assert mine == getattr(rev, l)() and len(mine) == counts[p]
            assert [k["name"] for k in mine] == [info(fwd, first + j)[0] for j in range(len(mine))], l
            first += len(mine)
        assert first == total
    finally:
        fwd.close(); rev.close()


def test_the_result_follows_the_current_theta(built):
    from infiniteexamodels.jl_amd.model import ExaModel
    core, blob, om, rows = model("shifted_pf")
    gm = ExaModel(core, device=0, blob=blob)
    try:
        x, y = point("shifted_pf", om)
        s = factors(om.ncon, "random")
        xd, yd, sd = _dev(x), _dev(y), _dev(s)

        def wit(o):
            return 0.3 * o.obj(x), s * o.cons(x), 0.3 * o.grad(x), s[rows] * o.jac_coord(x), o.hess_coord(x, y * s, 0.21)

        def got():
            f, c = gm.eval_trial_scaled(xd, sd, 0.3, _poisoned(om.ncon))
            g, jac, hess = gm.eval_accepted_scaled(xd, yd, sd, 0.3, _poisoned(om.nvar), _poisoned(om.nnzj), _poisoned(om.nnzh), obj_weight=0.7)
            return np.array([f]), c.cpu().numpy(), g.cpu().numpy(), jac.cpu().numpy(), hess.cpu().numpy()
        before = wit(om)
        assert max(rel(a, np.asarray(b).reshape(a.shape)) for a, b in zip(got(), before)) <= TOL
        th2 = np.asarray(core.theta) * 1.1 + 0.05
        om2 = OracleModel(blob)
        om2.set_parameter(0, th2)
        after = wit(om2)
        assert max(rel(np.asarray(a), np.asarray(b)) for a, b in zip(after, before)) > 1e-6      # the check can tell, by the witness alone
        gm.set_parameter(0, th2)
        assert max(rel(a, np.asarray(b).reshape(a.shape)) for a, b in zip(got(), after)) <= TOL
    finally:
        gm.close()


def test_phases_are_capturable_and_the_objective_can_be_deferred(built):
    """scaled_phase_prepare() does the synchronous set-up.  One capture of eval_accepted_scaled and one of the trial phase's
    launch, replayed with new x, y, s in the same buffers: each replay bitwise the direct call.  Of the captured trial launch
    only its device-side part is taken, the constraints: the objective's slot is armed and read on the host, so the value is
    collected outside the capture, by an uncaptured call (the header's rule for the deferred form).  Then the deferred
    objective: obj_end returns the SCALED value, a following unscaled eval_trial the unscaled one."""
    import torch
    from infiniteexamodels.jl_amd.model import ExaModel
    name = "quadrotor_1000"
    core, blob, om, rows = model(name)
    gm = ExaModel(core, device=0, blob=blob)
    try:
        assert gm.scaled_phase_prepare() == 7
        x, y = point(name, om)
        xd, yd, sd = _dev(x), _dev(y), _dev(factors(om.ncon, "random"))
        g, jac, hess, c = _poisoned(om.nvar), _poisoned(om.nnzj), _poisoned(om.nnzh), _poisoned(om.ncon)
        gm.eval_accepted_scaled(xd, yd, sd, 0.3, g, jac, hess, obj_weight=0.7)      # (warm: nothing is set up inside the capture)
        gm.eval_trial_scaled(xd, sd, 0.3, c)
        torch.cuda.synchronize()
        ga, gt = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(ga):
            gm.eval_accepted_scaled(xd, yd, sd, 0.3, g, jac, hess, obj_weight=0.7)
        with torch.cuda.graph(gt):
            gm.eval_trial_scaled(xd, sd, 0.3, c, defer_obj=True)
        gm.obj_end()      # (disarms the slot the capture armed; nothing ran, the value is not one)
        for seed in (1, 2, 3):
            x2, y2 = point(name, om, seed)
            xd.copy_(_dev(x2)); yd.copy_(_dev(y2)); sd.copy_(_dev(factors(om.ncon, "random", seed)))
            for t in (g, jac, hess):
                t.fill_(float("nan"))
            ga.replay()
            torch.cuda.synchronize()
            want = gm.eval_accepted_scaled(xd, yd, sd, 0.3, _poisoned(om.nvar), _poisoned(om.nnzj), _poisoned(om.nnzh), obj_weight=0.7)
            assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip((g, jac, hess), want))
            assert rel(hess.cpu().numpy(), om.hess_coord(x2, y2 * sd.cpu().numpy(), 0.21)) <= TOL
            c.fill_(float("nan"))
            gt.replay()
            torch.cuda.synchronize()
            assert torch.equal(_bits(c), _bits(gm.cons_scaled(xd, sd, _poisoned(om.ncon))))
            # the trial point outside a capture, its objective deferred
            none, c2 = gm.eval_trial_scaled(xd, sd, 0.3, _poisoned(om.ncon), defer_obj=True)
            assert none is None
            f = gm.obj_end()
            f0 = gm.obj(xd)
            assert _fbits(f) == _fbits(0.3 * f0) and f != f0
            assert torch.equal(_bits(c2), _bits(gm.cons_scaled(xd, sd, _poisoned(om.ncon))))
            none, _ = gm.eval_trial(xd, defer_obj=True)      # every arm resets the factor: the unscaled value, untouched
            assert _fbits(gm.obj_end()) == _fbits(f0)
            gm.obj_begin(xd)
            assert _fbits(gm.obj_end()) == _fbits(f0)
    finally:
        gm.close()


def test_member_launch_fallback(built):
    """phase_kernels = 0: neither program has a phase kernel, the two calls make the member launches — the same bytes"""
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.model import ExaModel
    name = "quadrotor_1000"
    core, blob, om, rows = model(name)
    gm = ExaModel(core, device=0, blob=blob)
    with iemlib.options(phase_kernels=0):
        g0 = ExaModel(core, device=0, blob=blob)
    try:
        assert {k["kind"] for k in g0.scaled_phase_kernels()} == {"cons", "jac", "hess", "obj", "grad"}
        assert {"trial", "accepted"} <= {k["kind"] for k in gm.scaled_phase_kernels()}
        x, y = point(name, om)
        xd, yd, sd = _dev(x), _dev(y), _dev(factors(om.ncon, "random"))
        fa, ca = g0.eval_trial_scaled(xd, sd, 0.3, _poisoned(om.ncon))
        fb, cb = gm.eval_trial_scaled(xd, sd, 0.3, _poisoned(om.ncon))
        assert _fbits(fa) == _fbits(fb) and torch.equal(_bits(ca), _bits(cb))
        a = g0.eval_accepted_scaled(xd, yd, sd, 0.3, _poisoned(om.nvar), _poisoned(om.nnzj), _poisoned(om.nnzh), obj_weight=0.7)
        b = gm.eval_accepted_scaled(xd, yd, sd, 0.3, _poisoned(om.nvar), _poisoned(om.nnzj), _poisoned(om.nnzh), obj_weight=0.7)
        assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(a, b))
        assert rel(a[0].cpu().numpy(), 0.3 * om.grad(x)) <= TOL
    finally:
        gm.close(); g0.close()


def test_nan_confinement(grid_mode):
    """The hand-built rows: the NaN row poisons exactly its own entries of c and jac and no Hessian entry outside its own; the
    gradient is NaN-free (the objective does not read the row)."""
    import torch
    from infiniteexamodels.jl_amd.model import ExaModel
    core, blob, om, rows = model(HAND)
    gm = ExaModel(core, device=0, blob=blob)
    try:
        x = CS.nan_point(om)
        _, y = point(HAND, om)
        s = factors(om.ncon, "random")
        nan_rows, _ = CS.rows_of()
        xd, yd, sd = _dev(x), _dev(y), _dev(s)
        f, c = gm.eval_trial_scaled(xd, sd, 0.3, _poisoned(om.ncon))
        g, jac, hess = (t.cpu().numpy() for t in gm.eval_accepted_scaled(xd, yd, sd, 0.3, _poisoned(om.nvar), _poisoned(om.nnzj), _poisoned(om.nnzh), obj_weight=0.7))
        c = c.cpu().numpy()
        assert np.isfinite(f) and np.array_equal(np.flatnonzero(np.isnan(c)), nan_rows)
        assert np.array_equal(np.unique(rows[np.isnan(jac)]), nan_rows) and np.isnan(jac).sum() == 2
        ynan = np.zeros(om.ncon); ynan[nan_rows] = np.nan
        mine = np.isnan(gm.hess_coord(xd, _dev(ynan), _poisoned(om.nnzh), obj_weight=0.0).cpu().numpy())
        assert mine.any() and not np.isnan(hess[~mine]).any()
        assert np.isfinite(g).all()
    finally:
        gm.close()


def test_sharded_handle_refuses(built):
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.model import ExaModel
    sm = ExaModel.sharded(cases.build_core("quadrotor_100").to_blob(), 1, 0, 2, device=0)
    try:
        z = lambda n: torch.zeros(n, dtype=torch.float64, device="cuda")
        x, s, y, c, g, j, h = z(sm.meta.nvar), z(sm.meta.ncon) + 1, z(sm.meta.ncon), z(sm.meta.ncon), z(sm.meta.nvar), z(sm.meta.nnzj), z(sm.meta.nnzh)
        L = iemlib.lib()
        n, f = C.c_int32(), C.c_double()
        p = lambda t: t.data_ptr()
        for what, call in (("iem_scaled_phase_prepare", lambda: L.iem_scaled_phase_prepare(sm._h, C.byref(n))),
                           ("iem_grad_scaled", lambda: L.iem_grad_scaled(sm._h, p(x), 0.5, p(g))),
                           ("iem_hess_coord_scaled", lambda: L.iem_hess_coord_scaled(sm._h, p(x), p(y), p(s), 1.0, p(h))),
                           ("iem_eval_trial_scaled", lambda: L.iem_eval_trial_scaled(sm._h, p(x), p(s), 0.5, p(c), C.byref(f))),
                           ("iem_eval_accepted_scaled", lambda: L.iem_eval_accepted_scaled(sm._h, p(x), p(y), p(s), 0.5, 1.0, p(g), p(j), p(h)))):
            assert call() == -4, what      # IEM_E_ARG
            msg = L.iem_last_error().decode()
            assert what in msg and "sharded" in msg and "out of scope" in msg, msg
        for call in (lambda: sm.scaled_phase_prepare(), lambda: sm.grad_scaled(x, 0.5), lambda: sm.eval_trial_scaled(x, s, 0.5),
                     lambda: sm.eval_accepted_scaled(x, y, s, 0.5), lambda: sm.hess_coord_scaled(x, y, s)):
            with pytest.raises(iemlib.IemError, match="sharded"):
                call()
        assert np.isfinite(sm.eval_trial(x)[0])      # (no refused call left the objective slot armed)
    finally:
        sm.close()


@pytest.mark.parametrize("name", [HAND, "quadrotor_1000"])
def test_scaled_model_phases_against_the_solver_side_scaling(name, built):
    """ScaledModel.eval_trial / eval_accepted against contrib.ipm._Scaled at a second point: c, jac and hess bitwise, g and f
    within 1e-10."""
    import torch
    from infiniteexamodels.jl_amd import scaling
    from infiniteexamodels.jl_amd.contrib.ipm import _Scaled
    from infiniteexamodels.jl_amd.model import ExaModel
    core, blob, om, rows = model(name)
    gm = ExaModel(core, device=0, blob=blob)
    try:
        x0 = _dev(np.asarray(om.x0, dtype=np.float64))
        mg = 0.5 * float(np.abs(om.jac_coord(np.asarray(om.x0, dtype=np.float64))).max())      # half the largest entry: some rows are scaled
        old = _Scaled(gm, x0, mg)
        sm = scaling.ScaledModel.at(gm, x0, max_gradient=mg)
        assert sm.obj_scale == old.df and torch.equal(_bits(sm.con_scale), _bits(old.dc))
        assert bool((sm.con_scale != 1.0).any())
        x = x0 + 0.05 * _dev(np.random.default_rng(3).random(om.nvar))
        y = _dev(np.random.default_rng(4).standard_normal(om.ncon))
        jac, hess = _poisoned(om.nnzj), _poisoned(om.nnzh)
        old.jac_hess_coord(x, y, jac, hess, obj_weight=0.7)
        f, c = sm.eval_trial(x, _poisoned(om.ncon))
        g, j2, h2 = sm.eval_accepted(x, y, _poisoned(om.nvar), _poisoned(om.nnzj), _poisoned(om.nnzh), obj_weight=0.7)
        assert torch.equal(_bits(c), _bits(old.cons(x))) and torch.equal(_bits(j2), _bits(jac)) and torch.equal(_bits(h2), _bits(hess))
        fo, go = old.obj(x), old.grad(x).cpu().numpy()
        assert abs(f - fo) <= TOL * max(1.0, abs(fo)) and rel(g.cpu().numpy(), go) <= TOL
        assert torch.equal(_bits(sm.grad(x)), _bits(g)) and torch.equal(_bits(sm.hess_coord(x, y, obj_weight=0.7)), _bits(hess))
        none, _ = sm.eval_trial(x, defer_obj=True)
        assert none is None and _fbits(sm.obj_end()) == _fbits(f)
    finally:
        gm.close()
