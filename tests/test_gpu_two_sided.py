"""GPU parity and reproducibility of models whose stencils reach to the RIGHT of their support (forward / central
differences, /root/reference/src/transform.jl:535; the heat workload's nested second derivative, transform.jl:141):
every entry point against the CPU oracle into poisoned outputs — indices equal, values within 1e-10 relative, the
bound of tests/test_gpu_parity.py — and ten repeated grad! / jtprod! / hprod! calls with identical bits, as
tests/test_gpu_determinism.py asks of the existing models."""
import numpy as np
import pytest

import cases_two_sided as C2

pytestmark = pytest.mark.gpu

RTOL = 1e-10


def _close(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, what
    if ref.size == 0:
        return
    assert np.isfinite(got).all(), f"{what}: non-finite values (an output slot was not written)"
    scale = np.maximum(np.abs(ref), 1e-10 * max(1.0, np.abs(ref).max()))
    err = np.abs(got - ref) / scale
    k = int(err.argmax())
    assert err[k] <= RTOL, f"{what}: rel err {err[k]:.3e} at {k} (got {got[k]!r}, ref {ref[k]!r})"


def _models(name):
    from infiniteexamodels.jl_amd.model import ExaModel
    from pyoracle import OracleModel
    core = C2.build_core(name)
    blob = core.to_blob()
    return OracleModel(blob), ExaModel(core, device=0, blob=blob)


@pytest.mark.parametrize("name", list(C2.MODELS))
def test_all_entry_points_match_oracle(name, grid_mode):
    import torch
    om, gm = _models(name)
    assert (gm.meta.nvar, gm.meta.ncon, gm.meta.nnzj, gm.meta.nnzh) == (om.nvar, om.ncon, om.nnzj, om.nnzh)
    for base in (0, 1):
        for a, b in ((gm.jac_structure(base), om.jac_structure(base)), (gm.hess_structure(base), om.hess_structure(base))):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    r, c = gm.jac_structure_device(0)
    assert np.array_equal(r.cpu().numpy(), om.jac_structure(0)[0]) and np.array_equal(c.cpu().numpy(), om.jac_structure(0)[1])
    r, c = gm.hess_structure_device(0)
    assert np.array_equal(r.cpu().numpy(), om.hess_structure(0)[0]) and np.array_equal(c.cpu().numpy(), om.hess_structure(0)[1])
    nan = lambda n: torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    for seed in (0, 7):
        x, y = C2.eval_point(om, seed)
        v, vc = np.random.default_rng(seed + 2).standard_normal(om.nvar), np.random.default_rng(seed + 3).standard_normal(om.ncon)
        xd, yd, vd, vcd = (torch.tensor(a, device="cuda") for a in (x, y, v, vc))
        f = gm.obj(xd)
        assert abs(f - om.obj(x)) <= RTOL * max(1.0, abs(om.obj(x)))
        _close(gm.cons(xd, nan(om.ncon)).cpu().numpy(), om.cons(x), "cons")
        _close(gm.grad(xd, nan(om.nvar)).cpu().numpy(), om.grad(x), "grad")
        _close(gm.jac_coord(xd, nan(om.nnzj)).cpu().numpy(), om.jac_coord(x), "jac")
        _close(gm.hess_coord(xd, yd, nan(om.nnzh), obj_weight=0.7).cpu().numpy(), om.hess_coord(x, y, 0.7), "hess")
        jv, hv = gm.jac_hess_coord(xd, yd, nan(om.nnzj), nan(om.nnzh), obj_weight=0.7)
        _close(jv.cpu().numpy(), om.jac_coord(x), "pair jac")
        _close(hv.cpu().numpy(), om.hess_coord(x, y, 0.7), "pair hess")
        _close(gm.jprod(xd, vd, nan(om.ncon)).cpu().numpy(), om.jprod(x, v), "jprod")
        _close(gm.jtprod(xd, vcd, nan(om.nvar)).cpu().numpy(), om.jtprod(x, vc), "jtprod")
        _close(gm.hprod(xd, yd, vd, nan(om.nvar), obj_weight=0.7).cpu().numpy(), om.hprod(x, y, v, 0.7), "hprod")
    gm.close()


@pytest.mark.parametrize("name", list(C2.MODELS))
def test_ten_calls_identical_bits(name, grid_mode):
    import torch
    om, gm = _models(name)
    x, y = C2.eval_point(om)
    v, vc = np.random.default_rng(2).standard_normal(om.nvar), np.random.default_rng(3).standard_normal(om.ncon)
    xd, yd, vd, vcd = (torch.tensor(a, device="cuda") for a in (x, y, v, vc))
    first = None
    for it in range(10):
        out = (gm.grad(xd).cpu().numpy().tobytes(), gm.jtprod(xd, vcd).cpu().numpy().tobytes(),
               gm.hprod(xd, yd, vd, obj_weight=0.7).cpu().numpy().tobytes())
        if first is None:
            first = out
        for a, b, what in zip(first, out, ("grad", "jtprod", "hprod")):
            assert a == b, f"{what} changed between call 0 and call {it}"
    gm.close()


def test_shard_halo_reports_both_directions(built):
    """`iem_shard_halo`: {halo_left, halo_right, reach_left, reach_right, doubles_to_right, doubles_to_left}.  A backward
    model reports {h, 0, 1, 0, d, 0} with h, d what `iem_shard_info` has always reported; central differences 1 / 1."""
    from infiniteexamodels.jl_amd import transcribe, workloads
    from infiniteexamodels.jl_amd.model import ExaModel
    q = transcribe.exa_core(workloads.quadrotor(40)).to_blob()
    for r in range(3):
        sm = ExaModel.sharded(q, 1, r, 3, device=0)
        info = sm.shard_info()
        assert list(sm.shard_halo().values()) == [info["halo"], 0, 1, 0, info["halo_doubles"], 0]
        assert info["halo"] == (1 if r else 0) and info["halo_doubles"] == 22
        sm.close()
    c = C2.build_core("central_1d").to_blob()
    for r in range(3):
        sm = ExaModel.sharded(c, 1, r, 3, device=0)
        assert list(sm.shard_halo().values()) == [1 if r else 0, 1 if r < 2 else 0, 1, 1, 5, 5]
        vm, vf = sm.shard_var_map()
        assert int(((vf & 8) != 0).sum()) == (5 if r < 2 else 0) and int(((vf & 4) != 0).sum()) == (5 if r else 0)
        # linear difference rows: jac_coord! / hess_coord! load no halo entry on either side and may carry the exchange,
        # cons! reads both sides and may not
        reads = sm.halo_reads()
        assert reads["cons"][0] and not reads["cons"][2]
        sm.close()
