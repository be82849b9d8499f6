"""The second-order correction of the filter line search (iem_soc_*, csrc/iem_soc_device.h) — what needs no device: the symbols and
the source of the code object (its own key, five kernels, no atomic, no inline assembly, no helpers, no scratch), the refusals that
come before any device work, the restatement (tests/soc_reference.py) against a second, literal transcription of Ipopt's
TrySecondOrderCorrection loop on a table of hand-built cases that reaches every branch, the corrected right-hand side through a host
solve on three models, and the Maratos effect on the test model `maratos`."""
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
import search_reference as sref
import soc_reference as cref
from test_gpu_search import DC, DW
from test_search import algorithm_a, as_dict, same

_HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = ("soc_open", "soc_rhs", "soc_trial", "soc_accept", "soc_select")
CALLS = ("iem_soc_create", "iem_soc_destroy", "iem_soc_open", "iem_soc_rhs", "iem_soc_trial", "iem_soc_accept", "iem_soc_select", "iem_soc_device", "iem_soc_state", "iem_soc_source")
RHS_MODELS = ["opf_7", "pandemic_20x3", "quadrotor_100"]


def test_symbols_and_bindings(built):
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.barrier import SecondOrderCorrection
    L = iemlib.lib()
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "iem.h")).read()
    for name in CALLS:
        assert name in iemlib.SYMBOLS and getattr(L, name).argtypes is not None and re.search(r"\bint " + name + r"\(", header), name
    assert C.sizeof(iemlib.SocOpts) == 24 and C.sizeof(iemlib.SocState) == 40
    assert iemlib.SocOpts._fields_[0][0] == "struct_size" and iemlib.SocState._fields_[0][0] == "struct_size"
    o = iemlib.SocOpts.defaults()
    assert {k: getattr(o, k) for k in cref.OPTS} == cref.OPTS == dict(max_soc=4, kappa_soc=0.99)      # Ipopt's defaults, stated twice
    for method in ("open", "rhs", "trial", "accept", "select", "state", "close", "__enter__", "__exit__", "__del__"):
        assert callable(getattr(SecondOrderCorrection, method)), method
    with pytest.raises(TypeError):
        iemlib.SocOpts.defaults(kappa=0.5)
    # the three "not there" sentences no longer name the correction
    root = os.path.join(os.path.dirname(__file__), "..")
    for doc in ("include/iem.h", "DESIGN.md", "README.md"):
        text = open(os.path.join(root, doc)).read()
        assert not re.search(r"inertia correction, the second-order\s+\**\s*correction", text), doc


def test_the_source(built):
    """a code object of its own with no helpers in front, compiled without contraction: the same text and key twice, the key fnv1a64
    of the text and neither the search object's nor a fixed object's (which still are the three they were), five kernels, no atomic,
    no inline assembly, no shared memory"""
    from infiniteexamodels.jl_amd import lib as iemlib
    src, key = iemlib.soc_source()
    assert iemlib.soc_source() == (src, key)
    h = 1469598103934665603
    for byte in src.encode():
        h = ((h ^ byte) * 1099511628211) & (2 ** 64 - 1)
    assert key == h
    fixed = list(iemlib.fixed_sources())
    assert [name for name, _, _ in fixed] == ["kkt_diag", "kkt_border", "barrier"] and key not in [k for _, _, k in fixed] + [iemlib.search_source()[1]]
    head = src.split("\n", 1)[0]
    assert head.startswith("// iem-flags:") and "-ffp-contract=off" in head
    prefix, own = src.split("// iem_soc_device.h", 1)
    assert "IEM_TILE" not in prefix and "iem_shared" not in src and prefix.count("\n") <= 5      # the prelude alone
    kernels = re.findall(r"__global__ [^\n]*void (\w+)\(", own)
    assert tuple(kernels) == KERNELS and src.count("__global__") == len(KERNELS)
    code = "\n".join(line.split("//", 1)[0] for line in own.splitlines())
    assert re.findall(r"\batomic\w*\(", code) == [] and "__hip_atomic" not in code and "asm" not in code and "__shared__" not in code
    # the search object's source does not know of it
    assert "soc_" not in iemlib.search_source()[0]


@pytest.mark.skipif(not os.path.exists(_HIPCC), reason="no hipcc")
def test_the_object_compiles_without_scratch(built, tmp_path):
    from infiniteexamodels.jl_amd import lib as iemlib
    src, _ = iemlib.soc_source()
    head = src.split("\n", 1)[0]
    hip = tmp_path / "s.hip"
    hip.write_text(src)
    p = subprocess.run([_HIPCC, "--genco", "--offload-arch=gfx950", *head[len("// iem-flags:"):].split(), "-Rpass-analysis=kernel-resource-usage",
                        "-o", str(tmp_path / "s.hsaco"), str(hip)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    usage, lds, cur = {}, {}, None
    for m in re.finditer(r"Function Name: (\S+)|ScratchSize \[bytes/lane\]: (\d+)|LDS Size \[bytes/block\]: (\d+)", p.stderr):
        if m.group(1):
            cur = m.group(1)
        elif m.group(2):
            usage[cur] = int(m.group(2))
        else:
            lds[cur] = int(m.group(3))
    assert usage == {k: 0 for k in KERNELS} and lds == {k: 0 for k in KERNELS}, (usage, lds)


def test_refusals_that_need_no_device(built):
    from infiniteexamodels.jl_amd import lib as iemlib
    L = iemlib.lib()
    err = lambda: L.iem_last_error().decode()
    N = None
    assert L.iem_soc_create(N, N, N) == -4 and "null" in err()
    assert L.iem_soc_destroy(N) == 0
    assert L.iem_soc_open(N) == -4 and "null" in err()
    assert L.iem_soc_state(N, N) == -4 and "null" in err()
    assert L.iem_soc_device(N, N) == -4 and "null" in err()
    assert L.iem_soc_rhs(N, *[N] * 8, 0.1, N) == -4 and "null" in err()
    assert L.iem_soc_rhs(N, *[N] * 8, -0.1, N) == -4 and "mu" in err()
    assert L.iem_soc_trial(N, *[N] * 7) == -4 and "null" in err()
    assert L.iem_soc_accept(N, N, N, N, 0.1, 1.0, N) == -4 and "null" in err()
    assert L.iem_soc_accept(N, N, N, N, float("nan"), 1.0, N) == -4 and "mu" in err()
    assert L.iem_soc_select(N, *[N] * 12) == -4 and "null" in err()


# ---- Ipopt's TrySecondOrderCorrection, a second time: scalars and a loop, written from BacktrackingLineSearch / FilterLSAcceptor -----
SOC_NAMES = dict(soc_state=cref.SOC_STATE, soc_rounds=cref.SOC_ROUNDS)


def soc_dict(ctl):
    return {**as_dict(ctl), **{k: sref.word(ctl, w) for k, w in SOC_NAMES.items()}, "alpha_prev": float(ctl[cref.SOC_ALPHA_PREV])}


def try_second_order_correction(c, filt, rounds, d_alpha, mu, sigma, o, so):
    """c: dict of the block's words by name behind the first trial; filt: list of (theta, phi); rounds: what the solve, the step and
    the evaluations give per round.  Returns (c, filt, d_alpha); soc_state ACTIVE where the table ends before the loop does."""
    c, filt, d_alpha = dict(c), list(filt), list(d_alpha)
    theta_curr, theta_trial = c["theta0"], c["theta_t"]
    # only behind the first (full) trial step of a search that goes on, and only where the step has not reduced the infeasibility
    if not (c["status"] == 0 and c["trials"] == 1) or not math.isfinite(theta_trial) or theta_curr > theta_trial:
        c["soc_state"] = cref.CLOSED
        return c, filt, d_alpha
    alpha_primal_test = c["alpha_max"]      # "the original step size" of the acceptance test
    alpha_primal_soc = c["alpha_max"]
    count_soc, theta_soc_old, accept, ran_out = 0, 0.0, False, False
    c["alpha_prev"] = alpha_primal_soc
    while count_soc < so["max_soc"] and not accept and (count_soc == 0 or theta_trial <= so["kappa_soc"] * theta_soc_old):
        theta_soc_old = theta_trial
        if count_soc == len(rounds):
            ran_out = True
            break
        # c_soc = alpha_primal_soc·c_soc + c(trial);  solve;  the fraction-to-the-boundary rule gives the new alpha_primal_soc
        c["alpha_prev"] = alpha_primal_soc
        (alpha_primal_soc, alpha_dual_soc), ft, (theta_new, sumlog) = rounds[count_soc]
        count_soc += 1
        if not alpha_primal_soc > 0.0:      # no step length: the correction is abandoned
            theta_trial = float("nan")
            break
        test = dict(c, alpha=alpha_primal_test, status=0, trials=0)
        got, got_filt, _ = algorithm_a(test, filt, ft, float(theta_new), float(sumlog), mu, sigma, dict(o, max_trials=2 ** 62, alpha_floor=0.0))
        c["phi_t"], c["theta_t"] = got["phi_t"], got["theta_t"]
        theta_trial = got["theta_t"]
        accept = got["status"] in (1, 2)
        if accept:
            filt = got_filt
            c.update(status=got["status"], count=got["count"], flags=got["flags"], alpha=alpha_primal_soc)
            d_alpha = [alpha_primal_soc, alpha_dual_soc]
    if ran_out or (not accept and count_soc == len(rounds) and count_soc < so["max_soc"] and theta_trial <= so["kappa_soc"] * theta_soc_old):
        c["soc_state"] = cref.ACTIVE
        c["alpha_prev"] = alpha_primal_soc
    else:
        c["soc_state"] = cref.ACCEPTED if accept else cref.CLOSED
    c["soc_rounds"] = count_soc
    return c, filt, d_alpha


def all_cases():
    return cref.cases(64) + [c for c in cref.cases(100) if "filter" in c[0]]


def test_the_restatement_against_ipopts_loop():
    seen = {}
    for case in all_cases():
        name, ctl, filt, rounds, o, so, want = case
        steps = cref.run_case(case)
        got_ctl, got_filt, got_alpha = steps[-1]
        g = soc_dict(got_ctl)
        for k, v in want.items():
            if k in ("state", "status", "rounds", "count"):
                assert g[dict(state="soc_state", status="status", rounds="soc_rounds", count="count")[k]] == v, (name, k, g)
            elif k == "overflow":
                assert bool(g["flags"] & 2) == v, name
        seen[name] = g
        if "preset" in want:      # decided before: open and every round leave every bit
            for s_ctl, s_filt, s_alpha in steps:
                assert np.array_equal(s_ctl.view(np.int64), steps[0][0].view(np.int64)) and np.array_equal(s_filt, filt, equal_nan=True) and list(s_alpha) == [0.0, 0.625], name
            continue
        count = sref.word(ctl, sref.COUNT)
        ref_c, ref_f, ref_alpha = try_second_order_correction(soc_dict(ctl), [tuple(r) for r in filt[:count]], [(tuple(a), ft, tuple(m)) for a, ft, m in rounds],
                                                              [0.0, 0.625], 0.1, 1.0, o, so)
        for k in g:
            if k == "alpha_prev" and g["soc_state"] != cref.ACTIVE:
                continue      # (word 15 is the last round's input; it has no reader once the correction is decided)
            assert same(g[k], ref_c[k]), (name, k, g, ref_c)
        assert [tuple(r) for r in got_filt[:g["count"]]] == ref_f, name
        assert list(got_alpha) == ref_alpha, (name, got_alpha, ref_alpha)
        # what a rejection must not touch, and what no round touches at all
        first = soc_dict(steps[0][0])
        if g["status"] == sref.SEARCHING:
            assert (g["alpha"], g["trials"], g["count"], g["flags"]) == (first["alpha"], first["trials"], first["count"], first["flags"]) and list(got_alpha) == [0.0, 0.625], name
            assert np.array_equal(got_filt, filt, equal_nan=True), name
        for k in ("alpha_max", "phi0", "theta0", "slope", "theta_min", "theta_max", "trials"):
            assert same(g[k], first[k]), (name, k)
        # a round behind the decision changes nothing
        if g["soc_state"] != cref.ACTIVE:
            again = cref.accept(got_ctl, got_filt, 9.0, np.array([1.0, 0.0]), np.array([0.75, 0.5]), got_alpha, 0.1, 1.0, o, so)
            assert np.array_equal(again[0].view(np.int64), got_ctl.view(np.int64)) and np.array_equal(again[1], got_filt, equal_nan=True) and list(again[2]) == list(got_alpha), name
            assert np.array_equal(cref.open_(got_ctl).view(np.int64), got_ctl.view(np.int64)), name      # open is idempotent
    must = ["not open: the first trial was accepted", "not open: the search failed (max_trials = 1)", "not open: UNUSABLE", "not open: two trials rejected",
            "not open: theta_t < theta0", "not open: theta_t NaN", "not open: theta_t inf", "open: theta_t == theta0", "accepted f-type in round 1",
            "f-type needs alpha_max in the switching condition", "accepted h-type by theta", "accepted h-type on a filter of 0", "accepted h-type on a filter of 63",
            "accepted h-type on a filter of 64", "accepted h-type on a filter of 65", "accepted h-type on a full filter", "rejected, continuing (theta 2.5 -> 2.4 -> 2.3)",
            "rejected by kappa_soc (theta 2.5 -> 2.49)", "rejected at max_soc = 4", "rejected at max_soc = 1", "unusable alpha_soc (+0.0)", "unusable alpha_soc (NaN) in round 2"]
    assert set(must) <= set(seen), set(must) - set(seen)
    assert {g["soc_state"] for g in seen.values()} == {cref.ACTIVE, cref.ACCEPTED, cref.CLOSED} and {g["status"] for g in seen.values()} >= {0, 1, 2, 3, 4}
    # the accepted step is alpha_soc's pair, the block's alpha is alpha_soc, not alpha_max
    ctl, _, d = cref.run_case(next(c for c in cref.cases(64) if c[0] == "accepted f-type in round 1"))[-1]
    assert list(d) == [0.75, 0.5] and ctl[sref.ALPHA] == 0.75 and ctl[sref.ALPHA_MAX] == 1.0 and sref.word(ctl, cref.SOC_ROUNDS) == 1


def test_grid_calls_restated():
    """the gates of rhs, trial and select; the two rounds of csoc; equality rows' slack entries never written"""
    P = bref.barrier_point("opf_7")
    B, st = P["B"], P["state"]
    n, m = len(st[0]), len(st[1])
    rng = np.random.default_rng(5)
    ct, s_t, rhs1, sol, ds = rng.standard_normal(m), np.where(B["eq"], np.nan, rng.standard_normal(m)), rng.standard_normal(n + m), rng.standard_normal(n + m), rng.standard_normal(m)
    poison, csoc0 = np.full(n + m, np.nan), rng.standard_normal(m)
    ine = ~B["eq"]
    act = sref.block(alpha_max=0.75, status=sref.SEARCHING, trials=1)
    sref.set_word(act, cref.SOC_STATE, cref.ACTIVE); act[cref.SOC_ALPHA_PREV] = 0.75
    r1, c1 = cref.rhs(B, act, st, P["c"], ct, s_t, rhs1, csoc0, poison)
    inf0 = np.where(B["eq"], P["c"] - B["ceq"], P["c"] - st[1])
    inf_t = np.where(B["eq"], ct - B["ceq"], ct - s_t)
    assert np.array_equal(c1, 0.75 * inf0 + inf_t) and np.array_equal(r1[:n], rhs1[:n]) and np.array_equal(r1[n:][B["eq"]], -c1[B["eq"]])
    _, dcon, rhs_first = bref.terms(B, st, P["r"], P["c"])
    # with csoc = c − s the corrected row is the first-order row
    z = sref.block(alpha_max=0.0); sref.set_word(z, cref.SOC_STATE, cref.ACTIVE)      # alpha_prev = 0: csoc = +0·prev + inf_t
    r0, _ = cref.rhs(B, z, st, P["c"], P["c"], st[1], rhs_first, csoc0, poison)
    assert np.array_equal(r0, rhs_first)
    act2 = act.copy(); sref.set_word(act2, cref.SOC_ROUNDS, 1); act2[cref.SOC_ALPHA_PREV] = 0.5
    _, c2 = cref.rhs(B, act2, st, P["c"], ct, s_t, rhs1, c1, poison)
    assert np.array_equal(c2, 0.5 * c1 + inf_t)
    bufs = (np.full(n, np.nan), np.full(m, np.nan))
    xt, st_new = cref.trial(B, act, st[0], st[1], sol, ds, np.array([0.25, 1.0]), bufs)
    assert np.array_equal(xt, st[0] + 0.25 * sol[:n]) and np.isnan(st_new[B["eq"]]).all() and np.array_equal(st_new[ine], (st[1] + 0.25 * ds)[ine])
    dirs_soc = tuple(rng.standard_normal(k) for k in (m, n, n, m, m))
    dirs = tuple(np.full(k, np.nan) for k in (m, n, n, m, m))
    for state in (cref.NONE, cref.ACTIVE, cref.ACCEPTED, cref.CLOSED):
        blk = act.copy(); sref.set_word(blk, cref.SOC_STATE, state)
        if state != cref.ACTIVE:
            r, c_ = cref.rhs(B, blk, st, P["c"], ct, s_t, rhs1, csoc0, poison)
            assert np.isnan(r).all() and np.array_equal(c_, csoc0)
            assert all(np.isnan(a).all() for a in cref.trial(B, blk, st[0], st[1], sol, ds, np.array([0.25, 1.0]), bufs))
        got_sol, got_dirs = cref.select(B, blk, sol, dirs_soc, poison, dirs)
        if state == cref.ACCEPTED:
            assert np.array_equal(got_sol, sol) and np.array_equal(got_dirs[1], dirs_soc[1]) and np.array_equal(got_dirs[2], dirs_soc[2])
            for k in (0, 3, 4):
                assert np.isnan(got_dirs[k][B["eq"]]).all() and np.array_equal(got_dirs[k][ine], dirs_soc[k][ine])
        else:
            assert np.isnan(got_sol).all() and all(np.isnan(d).all() for d in got_dirs)
    for a in (0.0, -1.0, np.nan):
        assert all(np.isnan(v).all() for v in cref.trial(B, act, st[0], st[1], sol, ds, np.array([a, 1.0]), bufs))


@pytest.mark.parametrize("name", RHS_MODELS)
def test_the_corrected_right_hand_side_solves_the_corrected_constraint(name, built):
    """rhs_soc through scipy's solve on the host matrix of tests/test_gpu_search.py's ladder (delta_w = 1e-2, delta_c = 1e-6) and the
    restated barrier_step: the corrected linearised constraint  J·dx − ds − delta_c·dy + csoc  (J·dx − delta_c·dy + csoc on equality
    rows) is met as well as the first-order system meets  J·dx − ds − delta_c·dy + (c − s): the same solver, the same norm — max |row|
    over max (|J||dx| + (|dy| + |rs|)·inv + delta_c·|dy| + |constant|) — with a margin of 4, for the two more rounded operations of csoc."""
    from scipy.sparse.linalg import splu
    P = bref.barrier_point(name)
    B, om, st = P["B"], P["om"], P["state"]
    n, m = om.nvar, om.ncon
    ine = ~B["eq"]
    sg, dcn, rh = bref.terms(B, st, P["r"], P["c"])
    K = dref.host_kkt_diag(om, st[0], st[2], sg, DW, dcn + DC)
    lu = splu(K.tocsc())
    _, J = bref.oracle_matrices(om, st[0], st[2])
    q = bref._side(B, st, bref.MU)
    nan3 = tuple(np.full(m, np.nan) for _ in range(3))

    def residual(rhs_vec, constant):
        sol = lu.solve(rhs_vec)
        dirs, alpha = bref.step(B, st, sol, nan3)
        dx, dy = sol[:n], sol[n:]
        ds = np.where(ine, dirs[0], 0.0)
        with np.errstate(all="ignore"):
            spread = np.where(ine, (np.abs(dy) + np.abs(q["rs"])) / q["sigs"], 0.0)
        res = J @ dx - ds - DC * dy + constant
        scale = abs(J) @ np.abs(dx) + spread + DC * np.abs(dy) + np.abs(constant)
        return float(np.abs(res).max()) / float(scale.max()), sol, dirs, alpha
    inf0 = np.where(B["eq"], P["c"] - B["ceq"], P["c"] - st[1])
    first, sol, dirs, alpha = residual(rh, inf0)
    # the rejected trial point of the full step, and one round of the correction
    xt = st[0] + alpha[0] * sol[:n]
    s_t = np.where(ine, st[1] + alpha[0] * dirs[0], np.nan)
    ct = om.cons(xt)
    ctl = sref.block(alpha=alpha[0], alpha_max=alpha[0], status=sref.SEARCHING, trials=1)
    sref.set_word(ctl, cref.SOC_STATE, cref.ACTIVE); ctl[cref.SOC_ALPHA_PREV] = alpha[0]
    rhs_soc, csoc = cref.rhs(B, ctl, st, P["c"], ct, s_t, rh, np.zeros(m), np.full(n + m, np.nan))
    assert np.array_equal(rhs_soc[:n], rh[:n]) and np.isfinite(rhs_soc).all() and not np.array_equal(rhs_soc[n:], rh[n:])
    second, sol_soc, _, alpha_soc = residual(rhs_soc, csoc)
    print(name, f"first-order residual {first:.3e}, corrected residual {second:.3e}, ratio {second / first:.3f}, alpha {alpha[0]:.3e}, alpha_soc {alpha_soc[0]:.3e}")
    assert second <= 4.0 * first
    assert not np.array_equal(sol_soc, sol)


def test_maratos_on_the_host():
    """x = (cos 0.8, sin 0.8) at every support, y = −1.5·w: the full Newton step is rejected with theta_t >= theta0 and round 1 of
    the correction is accepted; the loop with the correction needs strictly fewer iterations and rejected trials than without"""
    P = cref.maratos_point()
    om, (x0, _, y0) = P["om"], P["state"][:3]
    assert np.allclose(sorted(P["weights"]), [0.25, 0.25, 0.5]) and np.array_equal(y0, -1.5 * P["weights"])
    logs = {True: [], False: []}
    with_soc = cref.host_loop(om, x0, y0, max_soc=4, log=logs[True].append)
    without = cref.host_loop(om, x0, y0, max_soc=0, log=logs[False].append)
    print("maratos, three supports, host: with the correction", {k: with_soc[k] for k in ("iterations", "rejected", "soc_accepted", "soc_rounds", "error")},
          "without", {k: without[k] for k in ("iterations", "rejected", "error")})
    first = with_soc["first"]
    assert first == dict(state=cref.ACCEPTED, status=sref.F_TYPE, rounds=1), first      # open went ACTIVE: rejected, theta_t >= theta0
    assert logs[False][0]["trials"] >= 1 and logs[True][0]["trials"] == 1 and logs[True][0]["alpha"] == 1.0
    for res in (with_soc, without):
        assert res["failed"] == 0 and res["error"] <= 1e-8
        xs = np.sort(res["x"])
        assert np.allclose(xs[:3], 0.0, atol=1e-7) and np.allclose(xs[3:], 1.0, atol=1e-7) and np.allclose(res["y"], -1.5 * P["weights"], atol=1e-6)
    assert with_soc["iterations"] < without["iterations"] and with_soc["rejected"] < without["rejected"] and with_soc["soc_accepted"] >= 1
    for angle, ys in ((0.8, 0.0), (1.5, -1.5)):      # the other two starts of the single-copy experiment: printed, and solved
        Q = cref.maratos_point(angle, ys)
        a, b = cref.host_loop(Q["om"], Q["state"][0], Q["state"][2], max_soc=4), cref.host_loop(Q["om"], Q["state"][0], Q["state"][2], max_soc=0)
        print(f"  start angle {angle}, y scale {ys}: with", (a["iterations"], a["rejected"], a["soc_accepted"]), "without", (b["iterations"], b["rejected"]))
        assert a["failed"] == 0 and a["error"] <= 1e-8 and b["failed"] == 0 and b["error"] <= 1e-8
