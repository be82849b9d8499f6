"""The hand-written code objects of one handle through their table (csrc/iem_api.cpp: kFixed, load_object) on the MI355X: the KKT
object with the border on the device, the per-row diagonal, the residual finishers and the barrier layer, all on ONE handle; then
everything destroyed, a second handle, and the same calls again — every output of the second pass carries the bits of the first.

The first pass meets the references of tests/test_gpu_kkt_diag.py and tests/test_gpu_barrier.py, with their helpers and their
tolerances: the inertia against the eigenvalues, the refined solve against the project's criterion (dref.residual_ok), the residual
and its norms bitwise against tests/kkt_diag_reference.py on iem_kktprod's output, a column of iem_kkt_solve_many bitwise
iem_kkt_solve on that column, sigma / dcon / rhs and the four maxima of the error block bitwise against tests/barrier_reference.py,
its four sums within (N + 2)·2⁻⁵²·Σ|term| of math.fsum.

farmer_5 has a dense border (iem_kkt_set_border(k, 1): kkt_border_ldl / kkt_border_solve run); quadrotor_5 has none and its chain
is the lane-per-row shape."""
import ctypes as C

import numpy as np
import pytest

import barrier_reference as bref
import kkt_diag_reference as dref
import test_gpu_barrier as tb
import test_gpu_kkt_diag as tk

pytestmark = pytest.mark.gpu
NRHS = 3


def one_pass(name):
    """every call on a fresh handle; returns the outputs as host arrays (NaN padding included) and what the checks need"""
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib
    P = bref.barrier_point(name)
    out = {}
    with tk.system(name, 1) as S:
        n, nvar = S.n, S.nvar
        rhs = tk.padded(S.B[:NRHS])
        tk.assemble_diag(S, S.dd)
        out["inertia"] = np.array(tk.factor(S))
        sol, norms = tk.refined_diag(S, S.dd, rhs, 1)
        # iem_kktprod's output per column of sol, for the reference's expression of the residual
        cols = sol[:, :n].contiguous()
        out["p"] = torch.stack([torch.cat(S.gm.kktprod(S.xd, S.yd, cols[u, :nvar].contiguous(), cols[u, nvar:].contiguous(), obj_weight=1.0)) for u in range(NRHS)]).cpu().numpy()
        S.gm._sync_stream()
        r, rnorms = tk.residual_diag(S, S.dd, rhs, sol)
        r1, n1 = tk.nan(n), tk.nan(1)      # iem_kkt_residual: the scalar delta_c, column 0
        S.check(S.L.iem_kkt_residual(S.k, tk._p(S.xd), tk._p(S.yd), 1.0, tk._p(S.sd), tk.DW, tk.DC, tk._p(S.B[0]), tk._p(cols[0]), tk._p(r1), tk._p(n1)))
        out.update(r1=r1, n1=n1)
        many = tk.solve_many(S, rhs)
        single = torch.stack([tk.solve(S, S.B[u]) for u in range(NRHS)])
        out.update(B=S.B[:NRHS], sol=sol, norms=norms, r=r, rnorms=rnorms, many=many, single=single)
        # the barrier layer on the same handle
        S.b = C.c_void_p()
        S.check(S.L.iem_barrier_create(S.gm._h, None, None, None, None, bref.RELAX, C.byref(S.b)))
        try:
            st = tuple(tb.dev(a) for a in P["state"])
            rr, cc = tb.dev(P["r"]), tb.dev(P["c"])
            out["sigma"], out["dcon"], out["rhs"] = tb.terms(S, st, rr, cc)
            out["error"] = tb.error(S, st, rr, cc)
            torch.cuda.synchronize()
        finally:
            S.check(S.L.iem_barrier_destroy(S.b))
        out = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in out.items()}
        info = iemlib.KktInfo()
        S.check(S.L.iem_kkt_info(S.k, C.byref(info)))
        out["ne"] = int(info.ne)
    return out


@pytest.mark.parametrize("name", ["farmer_5", "quadrotor_5"])
def test_two_handles_same_bits_and_the_references(name, built):
    h, P = dref.host_system(name), bref.barrier_point(name)
    B = P["B"]
    nvar, ncon = h["om"].nvar, h["om"].ncon
    n = nvar + ncon
    first = one_pass(name)
    second = one_pass(name)
    assert set(first) == set(second)
    for key in first:
        a, b = np.asarray(first[key]), np.asarray(second[key])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), key
    assert (first["ne"] > 0) == (name == "farmer_5")
    # the KKT object: the references of tests/test_gpu_kkt_diag.py
    inertia = first["inertia"]
    print(name, "n", n, "border", first["ne"], "inertia", inertia.tolist(), "eigenvalues", h["neg"])
    assert inertia[2] == 0 and inertia[0] + inertia[1] == n and inertia[1] == h["neg"]
    rhs, sol = first["B"], first["sol"][:, :n]
    assert tb.same_bits(rhs[0], h["rhs"])
    assert np.isnan(first["sol"][:, n:]).all() and np.isnan(first["r"][:, n:]).all() and np.isnan(first["many"][:, n:]).all()
    for u in range(NRHS):
        ok, resid, comp = dref.residual_ok(h["K"], sol[u], rhs[u])
        print(name, "column", u, "residual after one step", resid, "componentwise", comp)
        assert ok, (name, u, resid, comp)
    want, want_nm = dref.residual_dm(first["p"], rhs, sol, h["sigma"], h["dcon"], tk.DW, tk.DC, nvar)
    assert tb.same_bits(first["r"][:, :n], want) and tb.same_bits(first["rnorms"], want_nm)
    assert tb.same_bits(first["rnorms"], np.abs(first["r"][:, :n]).max(axis=1))
    want, want_nm = dref.residual_dm(first["p"][:1], rhs[:1], sol[:1], h["sigma"], None, tk.DW, tk.DC, nvar)      # without dcon: iem_kkt_residual
    assert tb.same_bits(first["r1"], want[0]) and tb.same_bits(first["n1"], want_nm)
    assert np.isfinite(first["norms"]).all() and tb.same_bits(first["norms"][1], first["rnorms"])      # the norms behind the step
    assert tb.same_bits(first["many"][:, :n], first["single"])
    # the barrier layer: the references of tests/test_gpu_barrier.py
    want = bref.terms(B, P["state"], P["r"], P["c"])
    for key, w, k in zip(("sigma", "dcon", "rhs"), want, (nvar, ncon, n)):
        assert np.isnan(first[key][k:]).all() and tb.same_bits(first[key][:k], w), key
    err = first["error"]
    head, *sums = bref.error(B, P["state"], P["r"], P["c"])
    assert np.isnan(err[8:]).all() and tb.same_bits(err[:4], head), (err[:4], head)
    for k, t in zip((4, 5, 6, 7), sums):
        w, bound = bref.sum_bound(t)
        print(name, f"out[{k}] = {err[k]!r}, fsum {w!r}, |difference| {abs(err[k] - w):.3e}, bound {bound:.3e}, terms {len(t)}")
        assert abs(err[k] - w) <= bound, k
