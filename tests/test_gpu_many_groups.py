"""Models over more than three infinite-parameter groups on the MI355X: every evaluation kind through
ExaModel.from_blob (the C-ABI) against the CPU oracle on the folded blob.  Bar as in
test_gpu_parity: structure bit-exact, values within 1e-10 relative."""
import warnings

import numpy as np
import pytest

import cases_many_groups as MG

pytestmark = pytest.mark.gpu

RTOL = 1e-10


def _close(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, what
    if ref.size == 0:
        return
    assert np.isfinite(got).all(), f"{what}: non-finite values"
    scale = np.maximum(np.abs(ref), 1e-10 * max(1.0, np.abs(ref).max()))
    err = np.abs(got - ref) / scale
    k = int(err.argmax())
    assert err[k] <= RTOL, f"{what}: rel err {err[k]:.3e} at {k} (got {got[k]!r}, ref {ref[k]!r})"


@pytest.fixture(scope="module")
def torch_cuda(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _blob(name):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return MG.build_core(name).to_blob()


def _check_all(gm, om, torch, seeds):
    assert (gm.meta.nvar, gm.meta.ncon, gm.meta.nnzj, gm.meta.nnzh) == (om.nvar, om.ncon, om.nnzj, om.nnzh)
    for base in (0, 1):
        for got, ref in ((gm.jac_structure(base), om.jac_structure(base)), (gm.hess_structure(base), om.hess_structure(base))):
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
        for got, ref in ((gm.jac_structure_device(base), om.jac_structure(base)),
                         (gm.hess_structure_device(base), om.hess_structure(base))):
            assert np.array_equal(got[0].cpu().numpy(), ref[0]) and np.array_equal(got[1].cpu().numpy(), ref[1])
    nanv = lambda n: torch.full((n,), float("nan"), device="cuda", dtype=torch.float64)
    out = []
    for seed in seeds:
        x, y = MG.eval_point(om, seed)
        xd, yd = torch.tensor(x, device="cuda"), torch.tensor(y, device="cuda")
        f = gm.obj(xd)
        assert abs(f - om.obj(x)) <= RTOL * max(1.0, abs(om.obj(x)))
        cv, gv, jv, hv = nanv(om.ncon), nanv(om.nvar), nanv(om.nnzj), nanv(om.nnzh)
        _close(gm.cons(xd, cv).cpu().numpy(), om.cons(x), "cons")
        _close(gm.grad(xd, gv).cpu().numpy(), om.grad(x), "grad")
        _close(gm.jac_coord(xd, jv).cpu().numpy(), om.jac_coord(x), "jac_coord")
        _close(gm.hess_coord(xd, yd, hv, obj_weight=0.3).cpu().numpy(), om.hess_coord(x, y, 0.3), "hess_coord")
        jv2, hv2 = nanv(om.nnzj), nanv(om.nnzh)
        gm.jac_hess_coord(xd, yd, jv2, hv2, obj_weight=0.3)
        assert torch.equal(jv2, jv) and torch.equal(hv2, hv), "fused jac + hess launch differs from the two calls"
        cv2 = nanv(om.ncon)
        f2, _ = gm.eval_trial(xd, cv2)
        assert f2 == f and torch.equal(cv2, cv), "iem_eval_trial differs from obj + cons!"
        gv2, jv3, hv3 = nanv(om.nvar), nanv(om.nnzj), nanv(om.nnzh)
        gm.eval_accepted(xd, yd, gv2, jv3, hv3, obj_weight=0.3)
        assert torch.equal(gv2, gv) and torch.equal(jv3, jv) and torch.equal(hv3, hv), "iem_eval_accepted differs"
        cv4, gv4, jv4, hv4 = nanv(om.ncon), nanv(om.nvar), nanv(om.nnzj), nanv(om.nnzh)
        f4 = gm.eval_all(xd, yd, cv4, gv4, jv4, hv4, obj_weight=0.3)[0]
        assert f4 == f and torch.equal(cv4, cv) and torch.equal(gv4, gv) and torch.equal(jv4, jv) and torch.equal(hv4, hv)
        gm.obj_begin(xd)
        gm.cons(xd, cv)
        assert gm.obj_end() == f
        rng = np.random.default_rng(seed + 40)
        v, vc = rng.standard_normal(om.nvar), rng.standard_normal(om.ncon)
        vd, vcd = torch.tensor(v, device="cuda"), torch.tensor(vc, device="cuda")
        _close(gm.jprod(xd, vd, nanv(om.ncon)).cpu().numpy(), om.jprod(x, v), "jprod")
        _close(gm.jtprod(xd, vcd, nanv(om.nvar)).cpu().numpy(), om.jtprod(x, vc), "jtprod")
        _close(gm.hprod(xd, yd, vd, nanv(om.nvar), obj_weight=0.3).cpu().numpy(), om.hprod(x, y, v, 0.3), "hprod")
        out.append((cv.cpu().numpy(), jv.cpu().numpy(), hv.cpu().numpy()))
    return out


@pytest.mark.parametrize("name", list(MG.many_group_cases()))
def test_every_kind_matches_oracle(name, torch_cuda, grid_mode):
    from infiniteexamodels.jl_amd.model import ExaModel
    from pyoracle import OracleModel
    blob = _blob(name)
    om = OracleModel(blob)
    gm = ExaModel.from_blob(blob, device=0)
    got1 = _check_all(gm, om, torch_cuda, (0, 7))
    gm.close()
    gm0 = ExaModel.from_blob(blob, device=0, options={"digit_fields": 0})   # the short columns gathered: the same bytes
    got0 = _check_all(gm0, om, torch_cuda, (0, 7))
    gm0.close()
    for a, b in zip(got1, got0):
        assert all(np.array_equal(u, v) for u, v in zip(a, b)), "digit_fields=0 differs from digit_fields=1"


def test_large_four_groups_matches_oracle(torch_cuda):
    from infiniteexamodels.jl_amd.model import ExaModel
    from pyoracle import OracleModel
    blob = _blob("large_four_groups")
    om = OracleModel(blob)
    assert om.ncon >= 100_000
    gm = ExaModel.from_blob(blob, device=0)
    _check_all(gm, om, torch_cuda, (0,))
    gm.close()


def test_chain_kkt_refuses(torch_cuda):
    from infiniteexamodels.jl_amd import kkt, kkt_chain
    from infiniteexamodels.jl_amd.model import ExaModel
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        core = MG.build_core("four_groups")
    gm = ExaModel(core, device=0)
    with pytest.raises(NotImplementedError):
        kkt_chain.ChainKKT(kkt.KKTSystem(gm))
    import ctypes as C
    from infiniteexamodels.jl_amd import lib as iemlib
    k = C.c_void_p()
    rc = gm._L.iem_kkt_create(gm._h, 0, C.byref(k))
    assert rc != 0 and b"chain KKT" in iemlib.lib().iem_last_error()
    gm.close()


def test_fresh_kernel_cache_compiles_with_hiprtc(torch_cuda, tmp_path, monkeypatch):
    """A 4-group model with the code-object cache pointed at an empty directory: generated, compiled
    at run time and evaluated equal to the oracle."""
    from infiniteexamodels.jl_amd.model import ExaModel
    from pyoracle import OracleModel
    monkeypatch.setenv("IEM_KERNEL_CACHE", str(tmp_path))
    blob = _blob("four_groups_b")
    om = OracleModel(blob)
    gm = ExaModel.from_blob(blob, device=0)
    _check_all(gm, om, torch_cuda, (3,))
    gm.close()
