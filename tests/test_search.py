"""The filter line search (iem_search_*, csrc/iem_search_device.h) — what needs no device: the symbols and the source of the code
object (its own key, three kernels, no atomic of its own, no inline assembly, no scratch), the refusals that come before any device
work, the restated acceptance test (tests/search_reference.py) against a second, literal scalar transcription of Algorithm A of
Waechter and Biegler 2006 on a table of hand-built cases that reaches every branch, and the restated slope terms against exact
arithmetic."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import barrier_reference as bref
import search_reference as sref

_HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = ("search_begin", "search_trial", "search_accept")
CALLS = ("iem_search_create", "iem_search_destroy", "iem_search_reset", "iem_search_begin", "iem_search_trial", "iem_search_accept", "iem_search_device",
         "iem_search_state", "iem_search_source")
SLOPE_MODELS = ["opf_7", "farmer_5", "pandemic_20x3", "quadrotor_100"]


def test_symbols_and_bindings(built):
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.barrier import FilterSearch
    L = iemlib.lib()
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "iem.h")).read()
    for name in CALLS:
        assert name in iemlib.SYMBOLS and getattr(L, name).argtypes is not None and re.search(r"\bint " + name + r"\(", header), name
    assert C.sizeof(iemlib.SearchOpts) == 80 and C.sizeof(iemlib.SearchState) == 112
    assert iemlib.SearchOpts._fields_[0][0] == "struct_size" and iemlib.SearchState._fields_[0][0] == "struct_size"
    o = iemlib.SearchOpts.defaults()
    assert {k: getattr(o, k) for k in sref.OPTS} == sref.OPTS      # Ipopt's defaults, stated twice
    for method in ("begin", "trial", "accept", "reset", "state", "close", "__enter__", "__exit__"):
        assert callable(getattr(FilterSearch, method)), method


def test_the_source(built):
    """a code object of its own behind the helpers of the device header, compiled without contraction: the same text and key twice,
    the key fnv1a64 of the text and none of the fixed objects', three kernels, no atomic but the tickets' (inside the helpers), no
    inline assembly — and iem_fixed_source still lists three"""
    from infiniteexamodels.jl_amd import lib as iemlib
    src, key = iemlib.search_source()
    assert iemlib.search_source() == (src, key)
    h = 1469598103934665603      # (the offset basis of the library's fnv1a64, as tests/test_fixed_objects.py states it)
    for byte in src.encode():
        h = ((h ^ byte) * 1099511628211) & (2 ** 64 - 1)
    assert key == h
    fixed = list(iemlib.fixed_sources())
    assert [name for name, _, _ in fixed] == ["kkt_diag", "kkt_border", "barrier"] and key not in [k for _, _, k in fixed]
    head = src.split("\n", 1)[0]
    assert head.startswith("// iem-flags:") and "-ffp-contract=off" in head
    # the same prelude and helper prefix as the barrier object: the texts agree up to their own kernels
    prefix, own = src.split("// iem_search_device.h", 1)
    assert prefix == iemlib.barrier_source()[0].split("// iem_barrier_device.h", 1)[0] and "#define IEM_TILE 256\n" in prefix
    kernels = re.findall(r"__global__ [^\n]*void (\w+)\(", own)
    assert tuple(kernels) == KERNELS and src.count("__global__") == len(KERNELS)      # none of the device header's own kernels
    code = "\n".join(line.split("//", 1)[0] for line in own.splitlines())
    assert re.findall(r"\batomic\w*\(", code) == [] and "__hip_atomic" not in code and "asm" not in code
    for helper in ("iem_shared_park<", "iem_shared_last(", "iem_shared_totals("):
        assert helper in code, helper
    assert "iem_grad_atomic(" not in code and "iem_grad_wave_uniform(" not in code and "iem_last_arrival" not in code


@pytest.mark.skipif(not os.path.exists(_HIPCC), reason="no hipcc")
def test_the_object_compiles_without_scratch(built, tmp_path):
    from infiniteexamodels.jl_amd import lib as iemlib
    src, _ = iemlib.search_source()
    head = src.split("\n", 1)[0]
    hip = tmp_path / "s.hip"
    hip.write_text(src)
    p = subprocess.run([_HIPCC, "--genco", "--offload-arch=gfx950", *head[len("// iem-flags:"):].split(), "-Rpass-analysis=kernel-resource-usage",
                        "-o", str(tmp_path / "s.hsaco"), str(hip)], capture_output=True, text=True)
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
    assert L.iem_search_create(N, N, N) == -4 and "null" in err()
    assert L.iem_search_destroy(N) == 0
    assert L.iem_search_reset(N) == -4 and L.iem_search_state(N, N) == -4 and L.iem_search_device(N, N, N) == -4
    assert L.iem_search_begin(N, *[N] * 8, 0.1, 1.0) == -4 and "null" in err()
    assert L.iem_search_begin(N, *[N] * 8, -0.1, 1.0) == -4 and "mu" in err()
    assert L.iem_search_trial(N, *[N] * 6) == -4 and "null" in err()
    assert L.iem_search_accept(N, N, N, 0.1, 1.0, N) == -4 and "null" in err()
    assert L.iem_search_accept(N, N, N, float("nan"), 1.0, N) == -4 and "mu" in err()


# ---- Algorithm A, a second time: scalars, lists and math.pow, written from the paper ------------------------------------------------
def algorithm_a(c, filt, ft, theta_t, sumlog, mu, sigma, o):
    """c: dict of the block's words by name; filt: list of (theta, phi).  Returns (c, filt, d_alpha[0])."""
    c, filt = dict(c), list(filt)
    if c["status"] in (1, 2):
        return c, filt, c["alpha"]
    if c["status"] in (3, 4):
        return c, filt, 0.0
    a, phi0, th0, m = c["alpha"], c["phi0"], c["theta0"], c["slope"]
    phi_t = sigma * ft - mu * sumlog
    c["phi_t"], c["theta_t"] = phi_t, theta_t
    in_filter = any(theta_t >= ft_ and phi_t >= fp_ for ft_, fp_ in filt)
    ok = not (math.isnan(phi_t) or math.isinf(phi_t) or math.isnan(theta_t) or math.isinf(theta_t)) and theta_t <= c["theta_max"] and not in_filter
    case_one = m < 0.0 and th0 <= c["theta_min"] and a * math.pow(-m, o["s_phi"]) > o["delta"] * math.pow(th0, o["s_theta"])      # (19)
    new_entry = ((1.0 - o["gamma_theta"]) * th0, phi0 - o["gamma_phi"] * th0)
    if ok and case_one:
        accepted = phi_t <= phi0 + o["eta_phi"] * a * m + 10.0 * 2.0 ** -52 * abs(phi0)      # (20)
        augment = False
        kind = 1
    elif ok:
        accepted = theta_t <= new_entry[0] or phi_t <= new_entry[1]      # (18)
        augment = accepted      # (22): the filter grows whenever (19) or (20) does not hold for the accepted step
        kind = 2
    else:
        accepted, augment, kind = False, False, 0
    if accepted:
        c["status"] = kind
        if augment:
            filt = [e for e in filt if not (e[0] >= new_entry[0] and e[1] >= new_entry[1])]
            if len(filt) < o["filter_capacity"]:
                filt.append(new_entry)
            else:
                c["flags"] |= 2
            c["count"] = len(filt)
        return c, filt, a
    c["trials"] += 1
    c["alpha"] = a / 2.0
    if c["trials"] == o["max_trials"] or c["alpha"] < o["alpha_floor"]:
        c["status"], c["alpha"] = 3, 0.0
    return c, filt, 0.0


NAMES = dict(alpha=sref.ALPHA, alpha_max=sref.ALPHA_MAX, phi0=sref.PHI0, theta0=sref.THETA0, slope=sref.SLOPE, theta_min=sref.THETA_MIN, theta_max=sref.THETA_MAX,
             phi_t=sref.PHI_T, theta_t=sref.THETA_T)
INTS = dict(status=sref.STATUS, trials=sref.TRIALS, count=sref.COUNT, flags=sref.FLAGS)


def as_dict(ctl):
    return {**{k: float(ctl[w]) for k, w in NAMES.items()}, **{k: sref.word(ctl, w) for k, w in INTS.items()}}


def same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def all_cases():
    out = sref.cases(64)
    for cap in (64, 100):
        for k in sref.filter_sizes(cap):
            out += sref.sized_case(k, cap)
    return out


def test_accept_against_algorithm_a():
    seen, switch = set(), set()
    for name, ctl, filt, ft, merit, mu, sigma, o, want in all_cases():
        count = sref.word(ctl, sref.COUNT)
        info = {}
        got_ctl, got_filt, got_alpha = sref.accept(ctl, filt, ft, merit, mu, sigma, o, info)
        ref_c, ref_f, ref_alpha = algorithm_a(as_dict(ctl), [tuple(r) for r in filt[:count]], ft, float(merit[0]), float(merit[1]), mu, sigma, o)
        g = as_dict(got_ctl)
        assert all(same(g[k], ref_c[k]) for k in g), (name, g, ref_c)
        assert [tuple(r) for r in got_filt[:g["count"]]] == ref_f, name
        assert got_alpha == ref_alpha and math.copysign(1.0, got_alpha) == 1.0, name
        assert np.array_equal(got_ctl[13:], np.zeros(3)) and np.array_equal(got_filt[max(g["count"], count):], filt[max(g["count"], count):], equal_nan=True), name
        # a one-ulp pow on the device cannot change a decision: the two sides of the comparison that involves pow are far apart
        if "switching_sides" in info:
            lhs, rhs = info["switching_sides"]
            assert abs(lhs - rhs) > 1e-12 * max(abs(lhs), abs(rhs)), (name, lhs, rhs)
            switch.add(lhs > rhs)
            if "switching" in want:
                assert (lhs > rhs) == want["switching"], name
        for k, v in want.items():
            if k == "status":
                assert g["status"] == v, (name, g)
            elif k == "count":
                assert g["count"] == v, (name, g)
            elif k == "overflow":
                assert bool(g["flags"] & 2) == v, name
        if g["status"] == sref.SEARCHING:
            assert g["trials"] == as_dict(ctl)["trials"] + 1 and g["alpha"] == 0.5 * float(ctl[sref.ALPHA]) and got_alpha == 0.0, name
        if sref.word(ctl, sref.STATUS) != sref.SEARCHING:      # decided already: nothing but d_alpha[0]
            assert np.array_equal(got_ctl.view(np.int64), ctl.view(np.int64)) and np.array_equal(got_filt, filt, equal_nan=True), name
        seen.add(name)
    must = ["f-type accepted", "f-type failing Armijo", "h-type accepted by theta", "h-type accepted by phi", "h-type rejected", "dominated by a filter entry",
            "theta_t > theta_max", "NaN phi_t", "inf theta_t", "max_trials reached", "alpha below the floor", "already accepted", "UNUSABLE", "filter append",
            "dominated entries removed with order kept", "filter full"]
    assert set(must) <= seen and switch == {True, False}
    # order kept: the survivors of the removal case are entries 0, 2, 5 of the six, then the new one
    name, ctl, filt, ft, merit, mu, sigma, o, _ = next(c for c in sref.cases(64) if c[0].startswith("dominated entries removed"))
    _, f2, _ = sref.accept(ctl, filt, ft, merit, mu, sigma, o)
    assert [tuple(r) for r in f2[:3]] == [tuple(filt[0]), tuple(filt[2]), tuple(filt[5])] and tuple(f2[3]) == ((1.0 - 1e-5) * 2.0, 10.0 - 1e-8 * 2.0)


def test_begin_restated():
    """the block of a first and a second begin, an unusable step length, a NaN slope"""
    err = np.array([0, 0, 0, 0, 0, 0, 3.0, -7.0])
    c0 = sref.block(status=sref.UNUSABLE)
    c1 = sref.begin(c0, -1.5, 4.0, err, np.array([0.75, 0.5]), 0.1, 2.0)
    d = as_dict(c1)
    assert d["alpha"] == d["alpha_max"] == 0.75 and d["phi0"] == 2.0 * 4.0 - 0.1 * -7.0 and d["theta0"] == 3.0 and d["slope"] == -1.5
    assert d["theta_min"] == 1e-4 * 3.0 and d["theta_max"] == 1e4 * 3.0 and d["status"] == 0 and d["trials"] == 0 and d["flags"] == 1 and math.isnan(d["phi_t"])
    err2 = err.copy(); err2[6] = 0.5
    d2 = as_dict(sref.begin(c1, -1.0, 4.0, err2, np.array([1.0, 1.0]), 0.1, 2.0))
    assert d2["theta_min"] == d["theta_min"] and d2["theta_max"] == d["theta_max"] and d2["theta0"] == 0.5
    assert as_dict(sref.begin(c0, -1.0, 4.0, err2, np.array([1.0, 1.0]), 0.1))["theta_min"] == 1e-4      # max(1, theta0)
    for slope, a in ((-1.0, 0.0), (float("nan"), 1.0)):
        d3 = as_dict(sref.begin(c1, slope, 4.0, err, np.array([a, 1.0]), 0.1))
        assert d3["status"] == sref.UNUSABLE and d3["alpha"] == 0.0 and d3["alpha_max"] == a


def search_point(name, seed=0):
    """the shared state of barrier_reference with what a search needs on top: grad f from the oracle and a random direction"""
    P = bref.barrier_point(name, seed)
    n, m = P["om"].nvar, P["om"].ncon
    rng = np.random.default_rng(77 + seed)
    return P, P["om"].grad(P["state"][0]), rng.standard_normal(n + m), rng.standard_normal(m)


@pytest.mark.parametrize("name", SLOPE_MODELS)
def test_slope_terms_against_exact_arithmetic(name, built):
    P, g, sol, ds = search_point(name)
    B, (x, s) = P["B"], P["state"][:2]
    mu, sigma = bref.MU, 0.75
    terms = sref.slope_terms(B, x, s, g, sol, ds, mu, sigma)
    assert len(terms) == len(x) + int((~B["eq"]).sum()) and np.isfinite(terms).all()
    F = Fraction
    exact = F(0)
    for i in range(len(x)):
        gb = (F(mu) / (F(B["xu"][i]) - F(x[i])) if B["hasU"][i] else 0) - (F(mu) / (F(x[i]) - F(B["xl"][i])) if B["hasL"][i] else 0)
        exact += (F(sigma) * F(g[i]) + gb) * F(sol[i])
    for j in np.nonzero(~B["eq"])[0]:
        gs = (F(mu) / (F(B["ru"][j]) - F(s[j])) if B["gU"][j] else 0) - (F(mu) / (F(s[j]) - F(B["rl"][j])) if B["gL"][j] else 0)
        exact += gs * F(ds[j])
    got = math.fsum(terms)
    bound = 8.0 * 2.0 ** -53 * math.fsum(np.abs(terms))
    print(name, f"slope {got!r}, |difference| {float(abs(F(got) - exact)):.3e}, bound {bound:.3e}, terms {len(terms)}")
    assert abs(F(got) - exact) <= F(bound)
    if name == "quadrotor_100":      # no bounds, no inequality rows: the terms are sigma·g·dx exactly
        assert B["counts"]["nz"] == 0 and np.array_equal(terms, (sigma * g) * sol[:len(x)])


def test_trial_restated():
    P, g, sol, ds = search_point("opf_7")
    B, (x, s) = P["B"], P["state"][:2]
    bufs = (np.full(len(x), np.nan), np.full(len(s), np.nan))
    xt, st = sref.trial(B, sref.block(alpha=0.25, status=sref.SEARCHING), x, s, sol, ds, bufs)
    assert np.array_equal(xt, x + 0.25 * sol[:len(x)]) and np.isnan(st[B["eq"]]).all() and np.array_equal(st[~B["eq"]], (s + 0.25 * ds)[~B["eq"]])
    for status in (sref.FAILED, sref.UNUSABLE):
        xt, st = sref.trial(B, sref.block(alpha=0.25, status=status), x, s, sol, ds, bufs)
        assert np.isnan(xt).all() and np.isnan(st).all()
