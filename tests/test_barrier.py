"""The interior-point barrier layer (iem_barrier_*, csrc/iem_barrier_device.h) — what needs no device: the symbols and bindings, the
source of the code object, the refusals that come before any device work, the host analysis (relaxed bounds, flags, counts) against
numpy, and THE ALGEBRA: the numpy restatement of the kernels (tests/barrier_reference.py) gives directions that satisfy the unreduced
primal-dual Newton system, and its start projection is contrib/ipm.py's push bit for bit."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import barrier_reference as bref
import kkt_diag_reference as dref

_HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = ("barrier_start", "barrier_terms", "barrier_step", "barrier_update", "barrier_error", "barrier_merit")
CALLS = ("iem_barrier_create", "iem_barrier_analyse", "iem_barrier_destroy", "iem_barrier_info", "iem_barrier_start", "iem_barrier_terms", "iem_barrier_step",
         "iem_barrier_update", "iem_barrier_error", "iem_barrier_merit", "iem_barrier_source")
ALGEBRA = ["opf_7", "pandemic_20x3", "farmer_5", "quadrotor_100", "test_problem_1"]
DW = 1e-2      # delta_w of the algebra test (delta_c = 0): part of the regularised Newton system the blocks state


def test_symbols_and_bindings(built):
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.barrier import BarrierLayer
    L = iemlib.lib()
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "iem.h")).read()
    for name in CALLS:
        assert name in iemlib.SYMBOLS and getattr(L, name).argtypes is not None and re.search(r"\bint " + name + r"\(", header), name
    assert C.sizeof(iemlib.BarrierInfo) == 88 and iemlib.BarrierInfo._fields_[0][0] == "struct_size"
    for method in ("start", "terms", "step", "update", "error", "merit", "optimality_error", "close", "__enter__", "__exit__"):
        assert callable(getattr(BarrierLayer, method)), method


def test_the_source(built, tmp_path):
    """a code object of its own behind the helpers of the device header (everything in front of its kernels), compiled without contraction: the six kernels,
    integer atomicMin / atomicMax as the only atomics of the new header, no float atomic, no scratch"""
    from infiniteexamodels.jl_amd import lib as iemlib
    src, key = iemlib.barrier_source()
    assert iemlib.barrier_source() == (src, key)
    head = src.split("\n", 1)[0]
    assert head.startswith("// iem-flags:") and "-ffp-contract=off" in head
    assert key not in (iemlib.kkt_border_source()[1], iemlib.kkt_diag_source()[1])
    own = src.split("// iem_barrier_device.h", 1)[1]
    for kernel in KERNELS:
        assert re.search(r"__global__ [^\n]*void " + kernel + r"\(", own), kernel
    code = "\n".join(line.split("//", 1)[0] for line in own.splitlines())
    assert set(re.findall(r"\batomic\w*\(", code)) == {"atomicMin(", "atomicMax("} and "asm" not in code
    assert src.count("__global__") == len(KERNELS)      # none of the device header's own kernels
    for helper in ("iem_shared_park<", "iem_shared_last(", "iem_shared_totals("):
        assert helper in code, helper
    assert "iem_grad_atomic(" not in code and "iem_grad_wave_uniform(" not in code and "iem_last_arrival" not in code
    if not os.path.exists(_HIPCC):
        return
    hip = tmp_path / "b.hip"
    hip.write_text(src)
    p = subprocess.run([_HIPCC, "--genco", "--offload-arch=gfx950", *head[len("// iem-flags:"):].split(), "-Rpass-analysis=kernel-resource-usage",
                        "-o", str(tmp_path / "b.hsaco"), str(hip)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    usage, cur = {}, None
    for m in re.finditer(r"Function Name: (\S+)|ScratchSize \[bytes/lane\]: (\d+)", p.stderr):
        if m.group(1):
            cur = m.group(1)
        else:
            usage[cur] = int(m.group(2))
    assert usage == {k: 0 for k in KERNELS}, usage


def test_refusals_that_need_no_device(built):
    from infiniteexamodels.jl_amd import lib as iemlib
    L = iemlib.lib()
    err = lambda: L.iem_last_error().decode()
    N = None
    assert L.iem_barrier_create(N, N, N, N, N, 1e-8, N) == -4 and "null" in err()
    assert L.iem_barrier_info(N, N) == -4 and L.iem_barrier_destroy(N) == 0
    assert L.iem_barrier_start(N, N, N, N, N, N, N, N, 1e-2, 1e-2) == -4 and "null" in err()
    assert L.iem_barrier_terms(N, *[N] * 9, 0.1, N, N, N) == -4 and "null" in err()
    assert L.iem_barrier_step(N, *[N] * 8, 0.1, 0.99, *[N] * 6) == -4 and "null" in err()
    assert L.iem_barrier_update(N, *[N] * 14, 0.1, 1e10) == -4 and "null" in err()
    assert L.iem_barrier_error(N, *[N] * 9, 0.1, N) == -4 and "null" in err()
    assert L.iem_barrier_merit(N, N, N, N, N) == -4 and "null" in err()
    # the scalars are judged first
    for tau in (0.0, -0.5, 1.5, float("nan")):
        assert L.iem_barrier_step(N, *[N] * 8, 0.1, tau, *[N] * 6) == -4 and "tau" in err(), tau
    for mu in (-1e-300, float("nan")):
        assert L.iem_barrier_terms(N, *[N] * 9, mu, N, N, N) == -4 and "mu" in err()
        assert L.iem_barrier_step(N, *[N] * 8, mu, 0.99, *[N] * 6) == -4 and "mu" in err()
        assert L.iem_barrier_update(N, *[N] * 14, mu, 1e10) == -4 and "mu" in err()
        assert L.iem_barrier_error(N, *[N] * 9, mu, N) == -4 and "mu" in err()
    assert L.iem_barrier_update(N, *[N] * 14, 0.1, 0.5) == -4 and "kappa_sigma" in err()
    assert L.iem_barrier_start(N, N, N, N, N, N, N, N, 0.0, 1e-2) == -4 and "bound_push" in err()
    # the refusals of create, through the host analysis
    inf = float("inf")
    ok = lambda **kw: iemlib.barrier_analyse(**{**dict(lvar=[0.0, -inf], uvar=[1.0, inf], lcon=[0.0, -inf], ucon=[0.0, 2.0], relax=1e-8), **kw})
    assert ok()[3]["nz"] == 3
    for kw, word in ((dict(relax=-1e-9), "relax"), (dict(relax=float("nan")), "relax"), (dict(lvar=[1.0, -inf], relax=0.0), "fixed"),
                     (dict(lcon=[-inf, -inf], ucon=[inf, 2.0]), "neither"), (dict(lvar=[2.0, -inf]), "lvar > uvar"), (dict(lcon=[0.0, 3.0]), "lcon > ucon")):
        with pytest.raises(iemlib.IemError, match=word):
            ok(**kw)
    assert ok(lvar=[1.0, -inf])[3]["n_xl"] == 1      # a fixed variable with relax > 0: an interval of twice the relaxation
    # struct_size: at most that many bytes are written
    info = iemlib.BarrierInfo()
    info.struct_size = 40
    info.n_xl = info.nz = -7
    b, f = np.zeros(10), np.zeros(4, dtype=np.uint8)
    a = [np.array(v) for v in ([0.0, -inf], [1.0, inf], [0.0, -inf], [0.0, 2.0])]
    assert L.iem_barrier_analyse(2, 2, *[v.ctypes.data for v in a], 1e-8, b.ctypes.data, f.ctypes.data, C.byref(info)) == 0
    assert (info.struct_size, info.nvar, info.ncon, info.n_eq, info.n_ineq, info.n_xl, info.nz) == (40, 2, 2, 1, 1, -7, -7)
    info.struct_size = 4
    assert L.iem_barrier_analyse(2, 2, *[v.ctypes.data for v in a], 1e-8, b.ctypes.data, f.ctypes.data, C.byref(info)) == -4 and "struct_size" in err()


@pytest.mark.parametrize("name", ["opf_7", "farmer_5", "pandemic_20x3", "quadrotor_100"])
def test_bound_relaxation_and_counts(name, built):
    from infiniteexamodels.jl_amd import lib as iemlib
    P = bref.barrier_point(name)
    B = P["B"]
    parts, fx, fc, info = iemlib.barrier_analyse(P["lvar"], P["uvar"], P["lcon"], P["ucon"], bref.RELAX)
    for k in ("xl", "xu", "rl", "ru", "ceq"):
        assert np.array_equal(parts[k], B[k]) and np.array_equal(np.signbit(parts[k]), np.signbit(B[k])), k
    assert np.array_equal(fx, B["hasL"] * 1 + B["hasU"] * 2) and np.array_equal(fc, B["gL"] * 1 + B["gU"] * 2 + B["eq"] * 4)
    n = info.pop("workgroups")
    assert info == B["counts"] and n == max(1, min(-(-(info["nvar"] + info["ncon"]) // 256), 4096))
    print(name, info)
    lv, uv, lc, uc = P["lvar"], P["uvar"], P["lcon"], P["ucon"]
    fin = np.isfinite
    if name == "opf_7":
        assert int((fin(lv) & fin(uv)).sum()) == 168 and int((lv == uv).sum()) == 8
        assert info["n_eq"] == 159 and int((~B["eq"] & ~fin(lc) & fin(uc)).sum()) == 48 and int((~B["eq"] & fin(lc) & fin(uc)).sum()) == 59
    if name == "farmer_5":
        assert int((fin(lv) & ~fin(uv)).sum()) == 30 and int((fin(lv) & fin(uv)).sum()) == 3
        assert info["n_eq"] == 0 and int((fin(lc) & ~fin(uc)).sum()) == 15 and int((~fin(lc) & fin(uc)).sum()) == 11
    if name == "quadrotor_100":
        assert info["nz"] == 0 and info["n_ineq"] == 0


@pytest.mark.parametrize("name", ALGEBRA)
def test_the_algebra(name, built):
    """sigma, dcon, rhs from the restated terms; K from kkt_diag_reference.host_kkt_diag, scipy's LU; the restated step: every block of
    the unreduced Newton system holds to 1e-9·max(1, ‖rhs‖∞, ‖sol‖∞)"""
    from scipy.sparse.linalg import splu
    P = bref.barrier_point(name)
    B, st, om = P["B"], P["state"], P["om"]
    sigma, dcon, rhs = bref.terms(B, st, P["r"], P["c"])
    assert np.isfinite(sigma).all() and np.isfinite(dcon).all() and np.isfinite(rhs).all() and (dcon[B["eq"]] == 0).all() and (dcon[~B["eq"]] > 0).all()
    K = dref.host_kkt_diag(om, st[0], st[2], sigma, DW, dcon + 0.0)
    sol = splu(K.tocsc()).solve(rhs)
    poison = tuple(np.full(om.ncon, bref.NAN) for _ in range(3))
    dirs, alpha = bref.step(B, st, sol, poison)
    for a in (dirs[0], dirs[3], dirs[4]):
        assert np.isnan(a[B["eq"]]).all() and np.isfinite(a[~B["eq"]]).all()
    blocks = bref.newton_blocks(P, bref.oracle_matrices(om, st[0], st[2]), sol, dirs, DW, 0.0)
    scale = max(1.0, np.abs(rhs).max(), np.abs(sol).max())
    worst = [float(np.abs(b).max()) if b.size else 0.0 for b in blocks]
    print(f"{name}: scale {scale:.3e}, blocks / scale {[w / scale for w in worst]}, alpha {alpha.tolist()}")
    assert max(worst) <= 1e-9 * scale, (worst, scale)
    assert 0.0 < alpha[0] <= 1.0 and 0.0 < alpha[1] <= 1.0
    if B["counts"]["nz"] == 0:
        assert alpha.tolist() == [1.0, 1.0] and (sigma == 0).all()
    # the update keeps the state interior and moves it; a zero step length moves nothing
    new = bref.update(B, st, sol, dirs, alpha)
    with np.errstate(invalid="ignore"):
        assert (new[0] > B["xl"]).all() and (new[0] < B["xu"]).all() and ((new[1] > B["rl"]) | B["eq"]).all() and ((new[1] < B["ru"]) | B["eq"]).all()
    assert not np.array_equal(new[0], st[0])
    bad = sol.copy(); bad[0] = bref.NAN      # a NaN in the direction: alpha_p = +0.0 whatever the bounds
    assert bref.step(B, st, bad, poison)[1][0] == 0.0
    same = bref.update(B, st, sol, dirs, np.array([0.0, alpha[1]]))
    assert all(np.array_equal(a.view(np.int64), b.view(np.int64)) for a, b in zip(same, st))


@pytest.mark.parametrize("name", ALGEBRA)
def test_start_is_the_push_of_contrib_ipm(name, built):
    """the restated barrier_start against the expressions of contrib/ipm.py:86-93 (torch on the CPU), bit for bit"""
    import torch
    P = bref.barrier_point(name)
    B, om = P["B"], P["om"]

    def push(v, lo, hi, has_lo, has_hi, k1=bref.PUSH, k2=bref.FRAC):      # contrib/ipm.py's, as it stands there
        both = has_lo & has_hi
        span = torch.where(both, hi - lo, torch.full_like(v, float("inf")))
        pl = torch.minimum(k1 * torch.clamp(lo.abs(), min=1.0), k2 * span)
        pu = torch.minimum(k1 * torch.clamp(hi.abs(), min=1.0), k2 * span)
        v = torch.where(has_lo, torch.maximum(v, lo + pl), v)
        return torch.where(has_hi, torch.minimum(v, hi - pu), v)
    T = torch.from_numpy
    rng = np.random.default_rng(2)
    # start points inside, on and far outside the bounds
    x0 = om.x0 + rng.standard_normal(om.nvar) * 10.0 ** rng.uniform(-3, 3, om.nvar)
    with np.errstate(invalid="ignore"):
        x0 = np.where(rng.random(om.nvar) < 0.2, np.where(B["hasL"], B["xl"], x0), x0)
        x0 = np.where(rng.random(om.nvar) < 0.2, np.where(B["hasU"], B["xu"], x0), x0)
    c = om.cons(P["state"][0]) + rng.standard_normal(om.ncon) * 10.0 ** rng.uniform(-3, 3, om.ncon)
    poison = tuple(np.full(om.ncon, bref.NAN) for _ in range(3))
    x, s, zL, zU, vL, vU = bref.start(B, x0, c, poison)
    want_x = push(T(x0), T(B["xl"]), T(B["xu"]), T(B["hasL"]), T(B["hasU"])).numpy()
    assert np.array_equal(x.view(np.int64), want_x.view(np.int64))
    ine = ~B["eq"]
    want_s = push(T(c[ine]), T(B["rl"][ine]), T(B["ru"][ine]), T(B["gL"][ine]), T(B["gU"][ine])).numpy()
    assert np.array_equal(s[ine].view(np.int64), want_s.view(np.int64)) and np.isnan(s[~ine]).all()
    assert np.array_equal(zL, B["hasL"] * 1.0) and np.array_equal(zU, B["hasU"] * 1.0)
    assert np.array_equal(vL[ine], B["gL"][ine] * 1.0) and np.array_equal(vU[ine], B["gU"][ine] * 1.0) and np.isnan(vL[~ine]).all() and np.isnan(vU[~ine]).all()
    with np.errstate(invalid="ignore"):
        assert (x > B["xl"]).all() and (x < B["xu"]).all() and (s[ine] > B["rl"][ine]).all() and (s[ine] < B["ru"][ine]).all()


def test_optimality_error_is_contrib_ipm_scaling():
    from infiniteexamodels.jl_amd.barrier import BarrierLayer
    out = [3.0, 5.0, 0.25, 7.0, 4.0e4, 6.0e4, 1.0, -2.0]
    m, nz = 100, 200
    sd = max(100.0, (out[4] + out[5]) / max(1, m + nz)) / 100.0
    sc = max(100.0, out[5] / max(1, nz)) / 100.0
    assert BarrierLayer.optimality_error(out, (m, nz)) == (max(5.0 / sd, 0.25, 7.0 / sc), 5.0 / sd, 0.25, 7.0 / sc)
    assert BarrierLayer.optimality_error([1.0, 0.0, 9.0, 9.0, 0.0, 0.0, 0.0, 0.0], (0, 0)) == (1.0, 1.0, 0.0, 0.0)
