"""The feasibility restoration phase (iem_resto_*, csrc/iem_resto_device.h) — what needs no device: the symbols and the source of
the code object (its own key, twelve kernels, no float atomic, no inline assembly of its own, no scratch), the refusals that come
before any device work, and the restatement (tests/resto_reference.py): its directions in the UNREDUCED primal-dual Newton system of
the restoration barrier problem on three models, the elastic start against the stationarity conditions of Ipopt's eq. (33), the slope
against a central finite difference of the restoration's barrier objective, the tables of hand-built return-test and filter-append
cases, and the host loop on the Waechter-Biegler family with and without the phase."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import barrier_reference as bref
import kkt_diag_reference as dref
import resto_reference as rref
import search_reference as sref

_HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = ("resto_enter", "resto_enter_filter", "resto_terms", "resto_step", "resto_merit", "resto_begin", "resto_trial", "resto_update", "resto_error", "resto_check",
           "resto_leave_max", "resto_leave")
CALLS = ("iem_resto_create", "iem_resto_destroy", "iem_resto_search", "iem_resto_enter", "iem_resto_terms", "iem_resto_step", "iem_resto_merit", "iem_resto_begin",
         "iem_resto_trial", "iem_resto_update", "iem_resto_error", "iem_resto_check", "iem_resto_leave", "iem_resto_device", "iem_resto_state", "iem_resto_source")
MODELS = ["opf_7", "pandemic_20x3", "quadrotor_100"]
DW = 1e-2


def test_symbols_and_bindings(built):
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.barrier import Restoration
    L = iemlib.lib()
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "iem.h")).read()
    for name in CALLS:
        assert name in iemlib.SYMBOLS and getattr(L, name).argtypes is not None and re.search(r"\bint " + name + r"\(", header), name
    assert C.sizeof(iemlib.RestoOpts) == 32 and C.sizeof(iemlib.RestoState) == 40
    o = iemlib.RestoOpts.defaults()
    assert {k: getattr(o, k) for k in rref.OPTS} == rref.OPTS == dict(rho=1000.0, kappa_resto=0.9, bound_mult_reset_threshold=1000.0)      # Ipopt's, stated twice
    for method in ("enter", "terms", "step", "merit", "begin", "trial", "update", "error", "check", "leave", "state", "device", "close", "__enter__", "__exit__"):
        assert callable(getattr(Restoration, method)), method
    with pytest.raises(TypeError):
        iemlib.RestoOpts.defaults(kappa=0.5)
    assert iemlib.RESTO_STATE == ("none", "active", "return")


def test_the_source(built):
    """a code object of its own behind the helpers of the device header, compiled without contraction: the same text and key twice,
    the key fnv1a64 of the text and no other object's, twelve kernels, no float atomic and no inline assembly in its own text"""
    from infiniteexamodels.jl_amd import lib as iemlib
    src, key = iemlib.resto_source()
    assert iemlib.resto_source() == (src, key)
    h = 1469598103934665603
    for byte in src.encode():
        h = ((h ^ byte) * 1099511628211) & (2 ** 64 - 1)
    assert key == h
    fixed = list(iemlib.fixed_sources())
    assert [name for name, _, _ in fixed] == ["kkt_diag", "kkt_border", "barrier"]
    assert key not in [k for _, _, k in fixed] + [iemlib.search_source()[1], iemlib.soc_source()[1]]
    head = src.split("\n", 1)[0]
    assert head.startswith("// iem-flags:") and "-ffp-contract=off" in head
    prefix, own = src.split("// iem_resto_device.h", 1)
    assert "#define IEM_TILE 256" in prefix and "iem_shared_park" in prefix and "__global__" not in prefix      # the helpers, none of the header's kernels
    kernels = re.findall(r"__global__ [^\n]*void (\w+)\(", own)
    assert tuple(kernels) == KERNELS and src.count("__global__") == len(KERNELS)
    code = "\n".join(line.split("//", 1)[0] for line in own.splitlines())
    assert set(re.findall(r"\batomic\w*\(", code)) == {"atomicMin(", "atomicMax("} and "asm" not in code and "iem_grad_atomic" not in code
    for other in (iemlib.search_source()[0], iemlib.soc_source()[0], fixed[2][1]):
        assert "resto_" not in other


@pytest.mark.skipif(not os.path.exists(_HIPCC), reason="no hipcc")
def test_the_object_compiles_without_scratch(built, tmp_path):
    from infiniteexamodels.jl_amd import lib as iemlib
    src, _ = iemlib.resto_source()
    head = src.split("\n", 1)[0]
    hip = tmp_path / "r.hip"
    hip.write_text(src)
    p = subprocess.run([_HIPCC, "--genco", "--offload-arch=gfx950", *head[len("// iem-flags:"):].split(), "-Rpass-analysis=kernel-resource-usage",
                        "-o", str(tmp_path / "r.hsaco"), str(hip)], capture_output=True, text=True)
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
    assert L.iem_resto_create(N, N, N) == -4 and "null" in err()
    bad = iemlib.RestoOpts.defaults(rho=0.0)
    assert L.iem_resto_create(N, C.byref(bad), N) == -4 and "null" in err()      # the object comes first: nothing of the options is read
    assert L.iem_resto_destroy(N) == 0
    assert L.iem_resto_search(N, N) == -4 and "null" in err()
    assert L.iem_resto_state(N, N) == -4 and "null" in err()
    assert L.iem_resto_device(N, N, N, N, N, N) == -4 and "null" in err()
    assert L.iem_resto_enter(N, *[N] * 8, 0.1) == -4 and "null" in err()
    assert L.iem_resto_enter(N, *[N] * 8, -0.1) == -4 and "mu" in err()
    assert L.iem_resto_terms(N, *[N] * 9, 0.1, 0.3, N, N, N) == -4 and "null" in err()
    assert L.iem_resto_terms(N, *[N] * 9, -0.1, 0.3, N, N, N) == -4 and "mu" in err()
    assert L.iem_resto_terms(N, *[N] * 9, 0.1, -0.3, N, N, N) == -4 and "zeta" in err()
    assert L.iem_resto_terms(N, *[N] * 9, 0.1, float("nan"), N, N, N) == -4 and "zeta" in err()
    assert L.iem_resto_step(N, *[N] * 8, 0.1, 0.99, 0.3, *[N] * 6) == -4 and "null" in err()
    for tau in (0.0, 1.5, float("nan")):
        assert L.iem_resto_step(N, *[N] * 8, 0.1, tau, 0.3, *[N] * 6) == -4 and "tau" in err()
    assert L.iem_resto_step(N, *[N] * 8, -1.0, 0.99, 0.3, *[N] * 6) == -4 and "mu" in err()
    assert L.iem_resto_merit(N, 0, N, N, N, 0.3, N) == -4 and "null" in err()
    assert L.iem_resto_merit(N, 2, N, N, N, 0.3, N) == -4 and "which" in err()
    assert L.iem_resto_merit(N, 0, N, N, N, -0.3, N) == -4 and "zeta" in err()
    assert L.iem_resto_begin(N, *[N] * 6, 0.1, 0.3) == -4 and "null" in err()
    assert L.iem_resto_begin(N, *[N] * 6, -0.1, 0.3) == -4 and "mu" in err()
    assert L.iem_resto_trial(N, *[N] * 6) == -4 and "null" in err()
    assert L.iem_resto_update(N, *[N] * 14, 0.1, 1e10) == -4 and "null" in err()
    assert L.iem_resto_update(N, *[N] * 14, 0.1, 0.5) == -4 and "kappa_sigma" in err()
    assert L.iem_resto_error(N, *[N] * 9, 0.1, 0.3, N) == -4 and "null" in err()
    assert L.iem_resto_error(N, *[N] * 9, 0.1, -0.3, N) == -4 and "zeta" in err()
    assert L.iem_resto_check(N, N, N, 0.1) == -4 and "null" in err()
    assert L.iem_resto_check(N, N, N, -0.1) == -4 and "mu" in err()
    assert L.iem_resto_leave(N, *[N] * 5) == -4 and "null" in err()


# ---- (a) the restated directions in the unreduced Newton system ------------------------------------------------------------------------
def direction(P, R, st, mu, zeta, tau=bref.TAU):
    """``(sigma, dcon, rhs, sol, dirs, alpha, R)`` of one restoration iteration at (P, R, st): the restated terms, scipy's LU on
    kkt_diag_reference.host_kkt_diag with the Hessian of y'c alone (obj_weight = 0) and one step of refinement, the restated step"""
    from scipy.sparse.linalg import splu
    B, om = P["B"], P["om"]
    r = om.jtprod(st[0], st[2])
    sigma, dcon, rhs = rref.terms(B, R, st, r, P["c"], mu, zeta)
    K = dref.host_kkt_diag(om, st[0], st[2], sigma, DW, dcon + 0.0, 0.0).tocsc()
    lu = splu(K)
    sol = lu.solve(rhs)
    sol = sol + lu.solve(rhs - K @ sol)
    poison = tuple(np.full(om.ncon, bref.NAN) for _ in range(3))
    dirs, alpha, R = rref.step(B, R, st, sol, poison, mu, tau, zeta)
    return sigma, dcon, rhs, sol, dirs, alpha, R


@pytest.mark.parametrize("name", MODELS)
def test_the_directions_solve_the_unreduced_system(name, built):
    """every block — stationarity in x, s, p, n, the row J·dx − ds − dp + dn, complementarity with the two extra rows — holds to
    1e-9·max(1, ‖rhs‖∞, ‖sol‖∞): the bound of tests/test_barrier.py for its own blocks"""
    P = bref.barrier_point(name)
    B, om = P["B"], P["om"]
    R, st, mu = rref.entered(P)
    zeta = math.sqrt(mu)
    sigma, dcon, rhs, sol, dirs, alpha, R = direction(P, R, st, mu, zeta)
    assert np.isfinite(sigma).all() and np.isfinite(dcon).all() and np.isfinite(rhs).all() and (dcon > 0).all()
    for a in (dirs[0], dirs[3], dirs[4]):
        assert np.isnan(a[B["eq"]]).all() and np.isfinite(a[~B["eq"]]).all()
    Q = dict(P, state=st)
    blocks = rref.newton_blocks(Q, R, bref.oracle_matrices(om, st[0], st[2], 0.0), sol, dirs, DW, 0.0, mu, zeta)
    scale = max(1.0, np.abs(rhs).max(), np.abs(sol).max())
    worst = [float(np.abs(b).max()) if b.size else 0.0 for b in blocks]
    print(f"{name}: mu {mu:.3e}, scale {scale:.3e}, blocks / scale {[w / scale for w in worst]}, alpha {alpha.tolist()}")
    assert max(worst) <= 1e-9 * scale, (worst, scale)
    assert 0.0 < alpha[0] <= 1.0 and 0.0 < alpha[1] <= 1.0
    # the update keeps p, n and their multipliers positive and moves them; a zero step length moves nothing
    new, R2 = rref.update(B, R, st, sol, dirs, alpha, mu)
    assert all((R2[k] > 0).all() for k in ("p", "n", "zp", "zn")) and not np.array_equal(R2["p"], R["p"])
    same, R3 = rref.update(B, R, st, sol, dirs, np.array([0.0, alpha[1]]), mu)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(same, st)) and all(np.array_equal(R3[k], R[k]) for k in rref.ROWS)
    same, R3 = rref.update(B, R, st, sol, dirs, np.array([alpha[0], 0.0]), mu)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(same, st)) and all(np.array_equal(R3[k], R[k]) for k in rref.ROWS)


# ---- (b) the elastic start -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS + ["wb_eq", "wb_ineq"])
def test_enter_is_stationary(name, built):
    """Ipopt's eq. (33): (p, n) minimise rho(p + n) − mu(ln p + ln n) on p − n = inf, i.e. p − n = inf and 2 rho = mu/p + mu/n.  To
    rounding: p = inf + n is one addition (half an ulp of p); n = h + root cancels where inf > 0 — its absolute error is at most
    4 ulps of |h| + root =: d — and mu/p + mu/n moves by (mu/p² + mu/n²)·d, plus 8 ulps of 2 rho for the divisions and the sum."""
    P = rref.point(name)
    B = P["B"]
    with np.errstate(invalid="ignore"):
        inf = rref.infeasibility(B, P["c"], P["state"][1])
    mu, rho = max(P["mu"], float(np.abs(inf).max())), rref.OPTS["rho"]
    R, st = rref.enter(B, rref.new_object(len(P["state"][0]), len(inf)), P["state"], P["c"], mu)
    p, n = R["p"], R["n"]
    assert (p > 0).all() and (n > 0).all() and np.array_equal(R["zp"], mu / p) and np.array_equal(R["zn"], mu / n)
    ulp = 2.0 ** -52
    assert (np.abs((p - n) - inf) <= ulp * (np.abs(p) + np.abs(n))).all()
    h = (mu - rho * inf) / (2.0 * rho)
    d = 4.0 * ulp * (np.abs(h) + np.sqrt(h * h + (mu * inf) / (2.0 * rho)))
    miss = np.abs(2.0 * rho - (mu / p + mu / n))
    bound = (mu / (p * p) + mu / (n * n)) * d + 8.0 * ulp * 2.0 * rho
    print(f"{name}: mu {mu:.3e}, worst stationarity miss / bound {float((miss / bound).max()):.3e}, largest bound {float(bound.max()):.3e}")
    assert (miss <= bound).all()
    # both conditions with the multiplier: lambda = rho − mu/p = mu/n − rho
    assert (np.abs((rho - mu / p) - (mu / n - rho)) <= bound).all()
    # the state: y = 0, present bound multipliers clipped at rho, absent ones and the slack side of equality rows as they were
    assert not st[2].any()
    for z0, z1, on in zip(P["state"][3:], st[3:], (B["hasL"], B["hasU"], B["gL"], B["gU"])):
        assert np.array_equal(z1[on], np.minimum(rho, z0[on])) and np.isnan(z1[~on]).all()
    assert np.array_equal(R["xR"], P["state"][0]) and (R["wx"] <= 1.0).all() and (R["wx"] > 0).all()
    assert not R["sR"][B["eq"]].any() and not R["ws"][B["eq"]].any()


# ---- (c) the slope -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
def test_the_slope_is_the_derivative_of_the_merit(name, built):
    """phi_R(t) = out[0] − mu·out[2] of resto_merit at (x, s, p, n) + t·(dx, ds, dp, dn), c held (it has no part in phi_R): the restated
    slope against (phi_R(h) − phi_R(−h))/(2h), h = 1e-6·alpha_primal.  The bound: the rounding of the difference, 8 ulps of the sum of
    |addends| of phi_R over 2h, plus the truncation h²/6·|phi_R'''| — phi_R is quadratic plus logarithms, the third derivative of
    −mu·log(gap + t·d) is 2 mu (d/gap)³ and |t d/gap| <= 1e-6 tau along the step, so the truncation is below 1e-12·sum |mu·d/gap|/3,
    covered by 1e-9·sum |slope terms|."""
    P = bref.barrier_point(name)
    B = P["B"]
    R, st, mu = rref.entered(P)
    zeta = math.sqrt(mu)
    _, _, _, sol, dirs, alpha, R = direction(P, R, st, mu, zeta)
    terms = rref.slope_terms(B, R, st, sol, np.where(B["eq"], 0.0, dirs[0]), mu, zeta)
    slope = math.fsum(terms)
    nvar = len(st[0])
    h = 1e-6 * float(alpha[0])

    def phi(t):
        x, s = st[0] + t * sol[:nvar], st[1] + t * dirs[0]
        Rt = dict(R, pt=R["p"] + t * R["dp"], nt=R["n"] + t * R["dn"])
        S0, S1, _, logs = rref.merit_terms(B, Rt, 1, x, s, P["c"])
        assert np.isfinite(logs).all()
        add = np.concatenate([rref.OPTS["rho"] * S0, (0.5 * zeta) * S1, -mu * logs])
        return math.fsum(add), math.fsum(np.abs(add))
    (up, a_up), (down, a_down) = phi(h), phi(-h)
    fd = (up - down) / (2.0 * h)
    bound = 8.0 * 2.0 ** -52 * (a_up + a_down) / (2.0 * h) + 1e-9 * math.fsum(np.abs(terms))
    print(f"{name}: slope {slope!r}, central difference {fd!r}, |difference| {abs(slope - fd):.3e}, bound {bound:.3e}")
    assert abs(slope - fd) <= bound


# ---- the tables ------------------------------------------------------------------------------------------------------------------------------
def test_the_return_test_cases():
    """every branch of resto_check, by a second statement of the rule on plain floats"""
    seen = set()
    for name, blk, ctl_o, filt_o, f, m, mu, want in rref.check_cases():
        got = rref.check(blk, ctl_o, filt_o, f, m, mu)
        assert int(got.view(np.int64)[rref.R_STATE]) == want, name
        state0 = int(blk.view(np.int64)[rref.R_STATE])
        if state0 != rref.ACTIVE:
            assert np.array_equal(got.view(np.int64), blk.view(np.int64)), name
            seen.add("gated")
            continue
        theta, phi = float(m[0]), f - mu * float(m[1])
        assert np.array_equal(got[[rref.R_THETA, rref.R_PHI]], [theta, phi], equal_nan=True), name
        cnt = sref.word(ctl_o, sref.COUNT)
        reasons = dict(nonfinite=not (math.isfinite(theta) and math.isfinite(phi)), reduction=not theta <= 0.9 * float(blk[rref.R_THETA_START]),
                       theta_max=not theta <= float(ctl_o[sref.THETA_MAX]), dominated=any(theta >= t and phi >= p for t, p in filt_o[:cnt]))
        assert (want == rref.RETURN) == (not any(reasons.values())), (name, reasons)
        seen.update(k for k, v in reasons.items() if v)
        seen.add("return" if want == rref.RETURN else "stay")
    assert seen == {"gated", "nonfinite", "reduction", "theta_max", "dominated", "return", "stay"}


def test_the_filter_append_cases():
    """resto_enter_filter is the h-type branch of search_accept: the same filter and count as search_reference.accept leaves for a trial
    point it accepts h-type from the same block"""
    for name, ctl_o, filt_o, count, overflow in rref.append_cases():
        blk, ctl, filt = rref.enter_filter(np.zeros(8), ctl_o, filt_o)
        assert sref.word(ctl, sref.COUNT) == count and bool(sref.word(ctl, sref.FLAGS) & 2) == overflow, name
        assert int(blk.view(np.int64)[rref.R_STATE]) == rref.ACTIVE and blk[rref.R_THETA_START] == ctl_o[sref.THETA0] and np.isnan(blk[2:4]).all()
        probe = ctl_o.copy()
        probe[sref.ALPHA] = 1.0
        sref.set_word(probe, sref.STATUS, sref.SEARCHING)
        sref.set_word(probe, sref.TRIALS, 0)
        got, got_filt, _ = sref.accept(probe, filt_o, 9.0, np.array([1.0, 0.0]), 0.1)      # theta 1 < (1 − 1e-5)·2: h-type
        assert sref.word(got, sref.STATUS) == sref.H_TYPE, name
        assert sref.word(got, sref.COUNT) == count and np.array_equal(got_filt[:count], filt[:count]) and sref.word(got, sref.FLAGS) == sref.word(ctl, sref.FLAGS), name
        words = [w for w in range(16) if w not in (sref.COUNT, sref.FLAGS)]
        assert np.array_equal(ctl.view(np.int64)[words], ctl_o.view(np.int64)[words]), name


def test_leave():
    P = bref.barrier_point("opf_7")
    B, st = P["B"], P["state"]
    blk = np.zeros(8)
    blk.view(np.int64)[0] = rref.RETURN
    small = tuple(np.where(np.isnan(a), a, np.minimum(a, 50.0)) if k >= 3 else a for k, a in enumerate(st))
    new, b2 = rref.leave(B, blk, small)
    assert not new[2].any() and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(new[3:], small[3:])) and int(b2.view(np.int64)[0]) == rref.NONE
    big = list(small)
    big[3] = small[3].copy()
    big[3][np.flatnonzero(B["hasL"])[0]] = 1000.5
    new, b2 = rref.leave(B, blk, tuple(big))
    for z, on in zip(new[3:], (B["hasL"], B["hasU"], B["gL"], B["gU"])):
        assert (z[on] == 1.0).all() and np.isnan(z[~on]).all()
    assert b2[rref.R_ZMAX] == 1000.5


# ---- (d), (e), (f) the host loop ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rref.WB_MODELS))
def test_the_host_loop_needs_the_phase(name, built):
    """without restoration the loop of tests/search_loop.py ends with a FAILED search; with it at least one restoration returns and the
    loop reaches the optimum: error <= 1e-8, |f / sum w − 1·optimum| relative 1e-6 (the weights of the trapezoid rule on [0, 1] sum to 1)"""
    from pyoracle import OracleModel
    om = OracleModel(rref.wb_core(name).to_blob())
    x0 = om.x0 if hasattr(om, "x0") else None
    without = rref.host_loop(om, x0, max_restorations=0)
    assert without["status"] == "search failed" and without["error"] > 1.0, without
    got = rref.host_loop(om, x0)
    print(name, {k: got[k] for k in ("status", "iterations", "error", "objective", "restorations", "resto_iterations")}, "without:", without["iterations"])
    optimum = rref.WB_MODELS[name]["optimum"]
    assert got["status"] == "solved" and got["restorations"] >= 1 and got["error"] <= 1e-8
    assert abs(got["objective"] / optimum - 1.0) <= 1e-6


def test_a_failed_restoration_is_reported(built):
    """a = −1, b = 0.5 from (−2, 3, 1): the search accepts tiny steps (there is no alpha_min rule), and the restoration entered from
    where it finally fails converges to a local minimiser of the infeasibility — reported, never "solved" """
    from infiniteexamodels.jl_amd import transcribe
    from pyoracle import OracleModel
    om = OracleModel(transcribe.exa_core(rref.wachter_biegler(-1.0, 0.5, 3, False, start=(-2.0, 3.0, 1.0))).to_blob())
    got = rref.host_loop(om)
    print({k: got[k] for k in ("status", "iterations", "error", "objective", "restorations", "resto_iterations", "why")})
    assert got["status"] == "restoration failed" and got["why"] in ("inner search failed", "no return within the cap") and got["error"] > 1e-8
