"""The explicit θ blocks in COO on the MI355X (iem_jacp_coord / iem_hessp_coord through model.ExaModel): coverage of
NaN-poisoned buffers with a guard behind them, the structure, the identities against the merged matrix-free kinds to the
derived bound of tests/param_coord_checks.py, the values ENTRY BY ENTRY against the dense blocks of torch autograd (θ a leaf,
1e-10 relative; one witness product per class of θ columns no row sees twice), bit-reproducibility, θ updates and the refusals.

The shapes are the smallest at which these kernels can still go wrong: shifted_pf(1100) — two full 512-lane workgroups
and a ragged tail, stencil-shifted θ reads, a finite parameter every item reads —, shifted_pf(150) below one workgroup,
the quadrotor at 600 supports, its collocation variant at the golden size, pfun / pfun_full, rosenbrock, the heat
workload at 20 x 21 (central) and the folded four-group model; both code shapes."""
import numpy as np
import pytest

import cases_param as CP
import param_coord_checks as PC
from pyoracle import OracleModel
from theta2_witness import WitnessTheta2

pytestmark = pytest.mark.gpu
TOL = 1e-10
GUARD = 64


def _core(name):
    from infiniteexamodels.jl_amd import transcribe, workloads
    if name == "shifted_pf_1100":
        return CP.shifted_pf(1100)
    if name == "quadrotor_600":
        return transcribe.exa_core(workloads.quadrotor(600))
    return CP.build_core(name)


NAMES = ["shifted_pf_1100", "shifted_pf", "quadrotor_600", "quadrotor_oc3_40", "pfun", "pfun_full", "rosenbrock", "heat_central",
         "four_groups_param"]
_ref = {}


def reference(name):
    """core, blob, oracle, autograd witness and the evaluation point: built once per model, shared, never changed"""
    if name not in _ref:
        core = _core(name)
        blob = core.to_blob()
        om = OracleModel(blob)
        x = om.x0 + 0.1 * np.random.default_rng(0).standard_normal(om.nvar)
        y = np.random.default_rng(1).standard_normal(om.ncon)
        _ref[name] = (core, blob, om, WitnessTheta2(core), x, y)
    return _ref[name]


def _nan(n):
    import torch
    return torch.full((n + GUARD,), float("nan"), dtype=torch.float64, device="cuda")


def _blocks(gm, xd, yd, sigma):
    """the three poisoned buffers after one jacp_coord + one hessp_coord"""
    nj, nx, npp = gm.param_coord_nnz()
    jb, xb, pb = _nan(nj), _nan(nx), _nan(npp)
    gm.jacp_coord(xd, vals=jb[:nj])
    gm.hessp_coord(xd, yd, obj_weight=sigma, vals_xp=xb[:nx], vals_pp=pb[:npp])
    return jb, xb, pb


def _products(gm, xd, yd, sigma):
    import torch
    t = lambda a: torch.tensor(a, device="cuda")
    return {"jpprod": lambda w: gm.jpprod(xd, t(w)).cpu().numpy(), "jptprod0": lambda yy: gm.jptprod(xd, t(yy), obj_weight=0.0).cpu().numpy(),
            "hpprod": lambda w: gm.hpprod(xd, yd, t(w), obj_weight=sigma).cpu().numpy(),
            "hptprod": lambda u: gm.hptprod(xd, yd, t(u), obj_weight=sigma).cpu().numpy(),
            "hppprod": lambda w: gm.hppprod(xd, yd, t(w), obj_weight=sigma).cpu().numpy()}


@pytest.mark.parametrize("name", NAMES)
def test_blocks_on_the_gpu(name, grid_mode):
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.model import ExaModel
    core, blob, om, A, x, y = reference(name)
    nvar, ncon, npar = om.nvar, om.ncon, om.npar
    gm = ExaModel(core, device=0, blob=blob)
    try:
        nnz = gm.param_coord_nnz()
        s0 = [gm.jacp_structure(), gm.hessxp_structure(), gm.hesspp_structure()]
        s1 = [gm.jacp_structure(1), gm.hessxp_structure(1), gm.hesspp_structure(1)]
        assert [len(r) for r, _ in s0] == list(nnz) and sum(nnz) > 0
        PC.check_structure(s0, s1, nvar, ncon, npar)
        for which, (r, c) in enumerate(s0):      # the blob-only path reports the handle's structure
            br, bc = iemlib.blob_param_coord_structure(blob, which)
            np.testing.assert_array_equal(br, r); np.testing.assert_array_equal(bc, c)
        hr, hc = gm.hess_structure()
        assert (hr >= hc).all()      # ... the triangle Hθθ shares with hess_structure
        xd, yd = torch.tensor(x, device="cuda"), torch.tensor(y, device="cuda")
        if name == "shifted_pf_1100":
            assert all(int(np.prod(k["grid"])) >= 3 for k in gm.param_coord_kernels())
        for sigma in (1.0, 0.0, -0.5):
            bufs = _blocks(gm, xd, yd, sigma)
            for b, n, what in zip(bufs, nnz, ("Jθ", "Hxθ", "Hθθ")):
                PC.check_coverage(b.cpu().numpy(), n, what)
            vals = tuple(b[:n].cpu().numpy() for b, n in zip(bufs, nnz))
            PC.check_identities(s0, vals, _products(gm, xd, yd, sigma), nvar, ncon, npar, np.random.default_rng(5))
            for _ in range(10):      # identical bits, call after call
                for a, b in zip(_blocks(gm, xd, yd, sigma), bufs):
                    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
        # values against autograd with θ a leaf
        sigma = 0.7
        jv, xv, pv = (b[:n].cpu().numpy() for b, n in zip(_blocks(gm, xd, yd, sigma), nnz))
        # ENTRY BY ENTRY: the dense blocks, a class of θ columns no row sees twice per witness product (param_coord_checks)
        worst = PC.check_entries(s0, (jv, xv, pv), {"jpprod": lambda v: A.jpprod(x, v), "hpprod": lambda v: A.hpprod(x, y, v, sigma),
                                                    "hppprod": lambda v: A.hppprod(x, y, v, sigma)}, nvar, ncon, npar, TOL)
        print(name, grid_mode, "nnz", nnz, "against autograd", worst)
        assert worst <= TOL
        # the kernels ran from the offline build and are listed last
        mine = gm.param_coord_kernels()
        assert mine and all(k["name"].startswith(("iem_jacp", "iem_hessp")) for k in mine)
        assert sum(k["alg_bytes_written"] for k in mine if k["kind"] == "jac") == 8 * nnz[0]
        assert sum(k["alg_bytes_written"] for k in mine if k["kind"] == "hess") == 8 * (nnz[1] + nnz[2])
        assert not any(k["jit"] for k in gm.kernels() + mine), "the blocks' program was compiled at run time: build() must precompile it"
        n_par, n_th2 = gm.param_prepare(), gm.hppprod_prepare()
        assert [k["name"] for k in gm._kernel_infos(gm.meta.n_kernels + n_par + n_th2, gm.meta.n_kernels + n_par + n_th2 + len(mine))] == [k["name"] for k in mine]
        # after set_parameter the values follow the new θ, the structure stays
        th2 = np.asarray(core.theta) * 1.1 + 0.05
        gm.set_parameter(0, th2)
        try:
            bufs = _blocks(gm, xd, yd, 1.0)
            vals = tuple(b[:n].cpu().numpy() for b, n in zip(bufs, nnz))
            PC.check_identities(s0, vals, _products(gm, xd, yd, 1.0), nvar, ncon, npar, np.random.default_rng(6))
            for (r, c), (r2, c2) in zip(s0, [gm.jacp_structure(), gm.hessxp_structure(), gm.hesspp_structure()]):
                np.testing.assert_array_equal(r, r2); np.testing.assert_array_equal(c, c2)
            if name.startswith("shifted_pf"):      # ... and the check can tell: these blocks depend on θ
                assert np.abs(vals[0] - jv).max() > 1e-6
        finally:
            gm.set_parameter(0, np.asarray(core.theta))
    finally:
        gm.close()


def test_one_null_output_and_wrong_lengths(built):
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.model import ExaModel
    core, blob, om, A, x, y = reference("shifted_pf")
    gm = ExaModel(core, device=0, blob=blob)
    try:
        xd, yd = torch.tensor(x, device="cuda"), torch.tensor(y, device="cuda")
        nj, nx, npp = gm.param_coord_nnz()
        L = iemlib.lib()
        assert L.iem_hessp_coord(gm._h, xd.data_ptr(), yd.data_ptr(), 1.0, None, None) == -4      # IEM_E_ARG
        assert "both outputs" in L.iem_last_error().decode()
        both = gm.hessp_coord(xd, yd)
        assert gm.hessp_coord(xd, yd, vals_pp=False)[1] is None and torch.equal(gm.hessp_coord(xd, yd, vals_pp=False)[0], both[0])
        assert torch.equal(gm.hessp_coord(xd, yd, vals_xp=False)[1], both[1])
        with pytest.raises(ValueError):
            gm.hessp_coord(xd, yd, vals_xp=False, vals_pp=False)
        only_x, only_p = _nan(nx), _nan(npp)
        iemlib.check(L.iem_hessp_coord(gm._h, xd.data_ptr(), yd.data_ptr(), 1.0, only_x.data_ptr(), None))
        iemlib.check(L.iem_hessp_coord(gm._h, xd.data_ptr(), yd.data_ptr(), 1.0, None, only_p.data_ptr()))
        assert torch.equal(only_x[:nx], both[0]) and torch.equal(only_p[:npp], both[1])
        assert torch.isnan(only_x[nx:]).all() and torch.isnan(only_p[npp:]).all()
        with pytest.raises(ValueError):
            gm.jacp_coord(xd, vals=torch.empty(nj + 1, dtype=torch.float64, device="cuda"))
        with pytest.raises(ValueError):
            gm.hessp_coord(xd, yd, vals_xp=torch.empty(nx + 1, dtype=torch.float64, device="cuda"))
        with pytest.raises(ValueError):
            gm.hessp_coord(xd, yd, vals_pp=torch.empty(npp + 1, dtype=torch.float64, device="cuda"))
        with pytest.raises(ValueError):
            gm.hessp_coord(xd[:-1], yd)
    finally:
        gm.close()


@pytest.mark.parametrize("name", CP.NO_PARAM)
def test_a_model_without_theta_launches_nothing(name, built):
    import torch
    from infiniteexamodels.jl_amd.model import ExaModel
    gm = ExaModel(CP.build_core(name), device=0)
    try:
        assert gm.param_coord_nnz() == (0, 0, 0)
        x = torch.tensor(gm.meta.x0, device="cuda")
        y = torch.ones(gm.meta.ncon, dtype=torch.float64, device="cuda")
        assert gm.jacp_coord(x).numel() == 0
        assert all(v.numel() == 0 for v in gm.hessp_coord(x, y))
        assert gm.param_coord_kernels() == []
    finally:
        gm.close()


def test_sharded_handle_refuses(built):
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd import transcribe, workloads
    from infiniteexamodels.jl_amd.model import ExaModel
    blob = transcribe.exa_core(workloads.quadrotor(4000)).to_blob()
    sm = ExaModel.sharded(blob, 1, 1, 2, device=0)
    try:
        x = torch.zeros(sm.meta.nvar, dtype=torch.float64, device="cuda")
        y = torch.zeros(sm.meta.ncon, dtype=torch.float64, device="cuda")
        L = iemlib.lib()
        assert L.iem_jacp_coord(sm._h, x.data_ptr(), x.data_ptr()) == -4      # IEM_E_ARG
        assert "iem_jacp_coord" in L.iem_last_error().decode() and "sharded" in L.iem_last_error().decode()
        assert L.iem_hessp_coord(sm._h, x.data_ptr(), y.data_ptr(), 1.0, x.data_ptr(), x.data_ptr()) == -4
        assert L.iem_param_coord_prepare(sm._h, None) == -4
        for call in (sm.param_coord_nnz, sm.jacp_structure, sm.hessxp_structure, sm.hesspp_structure):
            with pytest.raises(iemlib.IemError, match="sharded"):
                call()
    finally:
        sm.close()
