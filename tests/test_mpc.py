"""Mehrotra's corrector's arithmetic and refusals without a GPU: tests/mpc_reference.py (the numpy restatement of
csrc/iem_mpc_device.h) against tests/barrier_reference.py, tests/amu_reference.py and the unreduced Newton system.

(a) symbols, struct sizes, the default stated twice, the refusals that need no device;
(b) the source: a code object of its own behind the helpers, the integer minimum its only atomic call, no scratch;
(c) with zero affine directions column 1 and the corrected step are barrier_reference.terms / step, bit for bit;
(d) the corrected direction solves the Newton system whose complementarity rows carry mu − dgap_aff·dz_aff;
(e) every branch of the decision;
(f) the restated loop with the corrector converges on the host, on a bounded linear model to the optimum of the plain probing loop."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import amu_reference as aref
import barrier_reference as bref
import mpc_reference as pref
import mu_reference as mref

_HIPCC = "/opt/rocm/bin/hipcc"
CALLS = ("iem_mpc_create", "iem_mpc_destroy", "iem_mpc_reset", "iem_mpc_bind_mu", "iem_mpc_terms", "iem_mpc_step", "iem_mpc_select", "iem_mpc_device",
         "iem_mpc_state", "iem_mpc_source")
KERNELS = ("mpc_reset", "mpc_select", "mpc_step", "mpc_terms")
DW = 1e-2      # delta_w of the Newton test (delta_c = 0), as in tests/test_barrier.py::test_the_algebra


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


def test_symbols_and_bindings(built):
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.barrier import MehrotraCorrector
    L = iemlib.lib()
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "iem.h")).read()
    for name in CALLS:
        assert name in iemlib.SYMBOLS and getattr(L, name).argtypes is not None and re.search(r"\bint " + name + r"\(", header), name
    assert C.sizeof(iemlib.MpcOpts) == 16 and C.sizeof(iemlib.MpcState) == 8 * 8
    assert iemlib.MpcOpts._fields_[0][0] == "struct_size" and iemlib.MpcState._fields_[0][0] == "struct_size"
    o = iemlib.MpcOpts.defaults()
    assert {k: getattr(o, k) for k in pref.OPTS} == pref.OPTS      # the default, stated twice
    for method in ("terms", "step", "select", "reset", "state", "device", "bind_mu", "close", "__enter__", "__exit__"):
        assert callable(getattr(MehrotraCorrector, method)), method
    with pytest.raises(TypeError):
        iemlib.MpcOpts.defaults(kappa=0.5)
    # the "Not here" lists of the sibling objects no longer name the corrector
    assert not re.search(r"Not here:[^/]*Mehrotra", header) and "Mehrotra's corrector is\n * not there" not in header


def test_the_source(built):
    """a code object of its own behind the helpers, compiled without contraction: the same text and key twice, the key fnv1a64 of the
    text and no other object's, its own four kernels only (terms, step, select among them), the integer minimum as the only atomic
    call of its own text, no inline assembly; no other object's source knows of it and the fixed sources are the three they were"""
    from infiniteexamodels.jl_amd import lib as iemlib
    src, key = iemlib.mpc_source()
    assert iemlib.mpc_source() == (src, key)
    h = 1469598103934665603
    for byte in src.encode():
        h = ((h ^ byte) * 1099511628211) & (2 ** 64 - 1)
    assert key == h
    fixed = list(iemlib.fixed_sources())
    assert len(fixed) == 3
    siblings = (iemlib.search_source, iemlib.soc_source, iemlib.resto_source, iemlib.mu_source, iemlib.barrier_mu_source, iemlib.amu_source, iemlib.qf_source)
    others = [k for _, _, k in fixed] + [f()[1] for f in siblings]
    assert key not in others and len(set(others)) == len(others)
    head = src.split("\n", 1)[0]
    assert head.startswith("// iem-flags:") and "-ffp-contract=off" in head
    prefix, own = src.split("// iem_mpc_device.h", 1)
    assert "#define IEM_TILE 256" in prefix
    kernels = re.findall(r"__global__ [^\n]*void (\w+)\(", own)
    assert tuple(sorted(kernels)) == KERNELS and src.count("__global__") == len(KERNELS)
    code = "\n".join(line.split("//", 1)[0] for line in own.splitlines())
    assert re.findall(r"\batomic\w*\(", code) == ["atomicMin("]      # ONE call site, on 64-bit integers: no atomicAdd on a float
    assert re.findall(r"__hip_atomic\w*", code) == ["__hip_atomic_load"]      # the relaxed look at the slot in front of it
    assert "atomicAdd" not in code and "asm" not in code and "cooperative" not in code and "grid.sync" not in code
    assert "iem_grad_atomic(" not in code and "iem_grad_wave_uniform(" not in code      # the helpers' float atomics stay unused
    for f in siblings + (iemlib.barrier_source,):
        assert "mpc_" not in f()[0]
    assert all("mpc_" not in text for _, text, _ in fixed)
    # the siblings keep their kernels
    assert iemlib.amu_source()[0].split("// iem_amu_device.h", 1)[1].count("__global__") == 3
    assert iemlib.qf_source()[0].split("// iem_qf_device.h", 1)[1].count("__global__") == 5


@pytest.mark.skipif(not os.path.exists(_HIPCC), reason="no hipcc")
def test_the_object_compiles_without_scratch(built, tmp_path):
    from infiniteexamodels.jl_amd import lib as iemlib
    src, _ = iemlib.mpc_source()
    head = src.split("\n", 1)[0]
    hip = tmp_path / "m.hip"
    hip.write_text(src)
    p = subprocess.run([_HIPCC, "--genco", "--offload-arch=gfx950", *head[len("// iem-flags:"):].split(), "-Rpass-analysis=kernel-resource-usage",
                        "-o", str(tmp_path / "m.hsaco"), str(hip)], capture_output=True, text=True)
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
    out = C.c_void_p()
    assert L.iem_mpc_create(N, N, C.byref(out)) == -4 and "null" in err()
    assert L.iem_mpc_create(N, C.byref(iemlib.MpcOpts.defaults()), N) == -4 and "null" in err()
    assert L.iem_mpc_destroy(N) == 0
    assert L.iem_mpc_reset(N) == -4 and "null" in err()
    assert L.iem_mpc_bind_mu(N, N) == -4 and "null" in err()
    assert L.iem_mpc_terms(N, *[N] * 15, 0.1, N, 0) == -4 and "null" in err()
    assert L.iem_mpc_step(N, *[N] * 14, 0.1, 0.99, *[N] * 6) == -4 and "null" in err()
    assert L.iem_mpc_select(N, *[N] * 15) == -4 and "null" in err()
    assert L.iem_mpc_device(N, N) == -4 and "null" in err()
    assert L.iem_mpc_state(N, N) == -4 and "null" in err()


# ---- (c) zero affine directions -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["opf_7", "farmer_5", "quadrotor_100", "test_problem_1"])
def test_zero_affine_directions_give_the_first_order_calls(name, built):
    """e = 0·0 = +0.0, m = mu ∓ 0 = mu: both columns are barrier_reference.terms, the corrected step barrier_reference.step, bit for bit"""
    P = bref.barrier_point(name)
    B, st = P["B"], P["state"]
    n, m = len(st[0]), len(st[1])
    zero_sol, zero_dirs = np.zeros(n + m), (np.zeros(m), np.zeros(n), np.zeros(n), np.zeros(m), np.zeros(m))
    for mu in (0.0, bref.MU):
        want = bref.terms(B, st, P["r"], P["c"], mu)[2]
        col0, col1 = pref.terms(B, st, P["r"], P["c"], zero_sol, zero_dirs, mu)
        assert np.array_equal(bits(col0), bits(want)) and np.array_equal(bits(col1), bits(want))
        sol, _, _ = aref.directions(P)
        poison = lambda: tuple(np.full(m, bref.NAN) for _ in range(3))
        dirs_w, alpha_w = bref.step(B, st, sol, poison(), mu, bref.TAU)
        dirs, alpha = pref.step(B, st, zero_sol, zero_dirs, sol, poison(), mu, bref.TAU)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(dirs, dirs_w)) and np.array_equal(bits(alpha), bits(alpha_w))


# ---- (d) the corrected Newton system --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["opf_7", "ode_5x5"])
def test_the_corrected_direction_solves_the_corrected_newton_system(name, built):
    """the affine direction, the two columns, scipy's LU of kkt_diag_reference.host_kkt_diag, the restated steps: every block of the
    unreduced Newton system holds to 1e-9·max(1, ‖rhs‖∞, ‖sol‖∞) — the tolerance of tests/test_barrier.py::test_the_algebra — for the
    first-order column with the target mu and for the corrected column with the target mu − dgap_aff·dz_aff; and the corrected
    column does NOT satisfy the uncorrected complementarity rows where a bound is present"""
    P = bref.barrier_point(name)
    B, st, om = P["B"], P["state"], P["om"]
    D = pref.corrected(P, bref.MU, DW)
    (sol_a, dirs_a, _), (sol0, dirs0, _), (sol1, dirs1, alpha1) = D["aff"], D["first"], D["corr"]
    K_parts = bref.oracle_matrices(om, st[0], st[2])
    for label, rhs, sol, blocks in (("first-order", D["rhs"][0], sol0, bref.newton_blocks(P, K_parts, sol0, dirs0, DW, 0.0)),
                                    ("corrected", D["rhs"][1], sol1, pref.newton_blocks(P, K_parts, sol_a, dirs_a, sol1, dirs1, DW, 0.0, bref.MU))):
        scale = max(1.0, np.abs(rhs).max(), np.abs(sol).max())
        worst = [float(np.abs(b).max()) if b.size else 0.0 for b in blocks]
        print(f"{name} {label}: scale {scale:.3e}, blocks / scale {[w / scale for w in worst]}")
        assert max(worst) <= 1e-9 * scale, (label, worst, scale)
    for a in (dirs1[0], dirs1[3], dirs1[4]):
        assert np.isnan(a[B["eq"]]).all() and np.isfinite(a[~B["eq"]]).all()
    if B["counts"]["nz"]:
        plain = bref.newton_blocks(P, K_parts, sol1, dirs1, DW, 0.0)[3]
        scale = max(1.0, np.abs(D["rhs"][1]).max(), np.abs(sol1).max())
        assert np.abs(plain).max() > 1e-6 * scale      # the second-order term is there
        assert 0.0 < alpha1[0] <= 1.0 and 0.0 < alpha1[1] <= 1.0


# ---- (e) the decision -----------------------------------------------------------------------------------------------------------------
def test_every_branch_of_the_decision(built):
    P = bref.barrier_point("opf_7")
    B, st = P["B"], P["state"]
    nz = B["counts"]["nz"]
    n, m = len(st[0]), len(st[1])
    rng = np.random.default_rng(3)
    vec = lambda k: rng.standard_normal(k)
    corrected = (vec(n + m), vec(m), vec(n), vec(n), vec(m), vec(m))
    first = tuple(vec(len(a)) for a in corrected)
    alpha, alpha_c = np.array([0.25, 0.5]), np.array([0.75, 0.875])
    ab = aref.fresh_block(aref.options())
    ab[aref.AVG] = 2.0
    opts = pref.options()
    cases_ = [("taken", [1.5 * nz, 0.0], alpha_c, B, opts), ("taken", [2.0 * nz, 0.0], alpha_c, B, opts),      # the bound itself is taken: <=
              ("NaN product", [1.5 * nz, 1.0], alpha_c, B, opts), ("NaN product", [1.5 * nz, np.nan], alpha_c, B, opts),
              ("zero step length", [1.5 * nz, 0.0], np.array([0.0, 0.5]), B, opts), ("zero step length", [1.5 * nz, 0.0], np.array([0.5, 0.0]), B, opts),
              ("average", [2.5 * nz, 0.0], alpha_c, B, opts), ("average", [np.nan, 0.0], alpha_c, B, opts),
              ("average", [1.5 * nz, 0.0], alpha_c, B, pref.options(red_fact=0.5)), ("taken", [2.5 * nz, 0.0], alpha_c, B, pref.options(red_fact=2.0)),
              ("nz = 0", [0.0, 0.0], alpha_c, dict(B, counts=dict(B["counts"], nz=0)), opts)]
    blk = pref.fresh_block()
    n_t = n_r = 0
    seen = set()
    for want, q, ac, Bc, o in cases_:
        probe = np.array([*q, ac[0], ac[1]])
        taken, predicted, reason = pref.decide(probe, ac, ab[aref.AVG], Bc["counts"]["nz"], o)
        assert reason == want and taken == (want == "taken"), (want, reason)
        seen.add(reason)
        blk, got, a = pref.select(Bc, blk, probe, ac, ab, o, corrected, first, alpha)
        n_t, n_r = n_t + taken, n_r + (not taken)
        iw = pref.ints(blk)
        assert (iw[pref.TAKEN], iw[pref.N_TAKEN], iw[pref.N_REFUSED]) == (int(taken), n_t, n_r)
        assert bits(blk[pref.PREDICTED]) == bits(predicted) and blk[pref.AVG] == 2.0 and np.array_equal(bits(blk[5:7]), bits(ac)) and not blk[7:].any()
        if taken:
            ine = ~B["eq"]
            assert np.array_equal(bits(got[0]), bits(corrected[0])) and np.array_equal(bits(got[2]), bits(corrected[2])) and np.array_equal(bits(got[3]), bits(corrected[3]))
            for k in (1, 4, 5):
                assert np.array_equal(bits(got[k][ine]), bits(corrected[k][ine])) and np.array_equal(bits(got[k][~ine]), bits(first[k][~ine]))
            assert np.array_equal(bits(a), bits(ac))
        else:
            assert all(np.array_equal(bits(g), bits(f)) for g, f in zip(got, first)) and np.array_equal(bits(a), bits(alpha))
    assert seen == set(pref.REASONS) and B["eq"].any() and (~B["eq"]).any()
    assert pref.decide(np.zeros(4), alpha_c, 2.0, 0, opts)[1] == 0.0      # nz = 0: predicted is +0.0, no division


# ---- (f) the loop on the host ---------------------------------------------------------------------------------------------------------
def _core(name):
    import cases
    from infiniteexamodels.jl_amd import transcribe
    if name == "rosenbrock":
        return transcribe.exa_core(cases.rosenbrock()[0])
    if name == "pfun":
        return transcribe.exa_core(cases.pfun()[0])
    return cases.build_core(name)


@pytest.mark.parametrize("name,want,iterations", [("rosenbrock", 306.4999755050365, (15, 16, 6, 10)), ("ode_5x5", -12.784599900757165, (8, 7, 7, 0))])
def test_the_restated_loop_converges_on_the_host(name, want, iterations, built):
    """mpc_reference.host_loop — the probing rule with the corrector, made of the restatements alone around a dense solve — reaches
    the optima the device loops are held to, to their tolerance, without a failed search.  The iteration counts without / with the
    corrector and the taken / refused counts of the host this was written on (rosenbrock 15 / 16, 6 taken, 10 refused by the
    average; ode_5x5 8 / 7, 7 taken, none refused) are printed beside what was found, not asserted."""
    from pyoracle import OracleModel
    om = OracleModel(_core(name).to_blob())
    plain = pref.host_loop(om, corrector=False)
    res = pref.host_loop(om, corrector=True)
    print(name, "iterations without / with", plain["iterations"], res["iterations"], "taken", res["taken"], "refused", res["refused"], "(written with", iterations, ")",
          "objective", repr(res["objective"]), "error", res["error"], {r: res["reasons"].count(r) for r in sorted(set(res["reasons"]))})
    assert res["failed"] == 0 and res["status"] == mref.CONVERGED and res["error"] <= 1e-8 and abs(res["objective"] - want) <= 1e-6
    assert res["taken"] + res["refused"] == len(res["reasons"]) and plain["taken"] == plain["refused"] == 0


def test_a_bounded_linear_model_on_the_host(built):
    """cases.pfun(): a linear objective, linear constraints, every variable in [0, 100] — the parameter-function LP of the
    reference's test/solve.jl.  (workloads.farmer at 5 scenarios is not used: the dense host loop does not converge on it with OR
    without the corrector — its search fails 8 times in both.)  The plain probing loop on the same host gives the optimum; the
    corrected loop agrees to 1e-6.  Written with: 11 iterations without, 10 with, 10 taken, none refused — printed, not asserted."""
    from pyoracle import OracleModel
    om = OracleModel(_core("pfun").to_blob())
    plain = pref.host_loop(om, corrector=False)
    res = pref.host_loop(om, corrector=True)
    print("pfun iterations without / with", plain["iterations"], res["iterations"], "taken", res["taken"], "refused", res["refused"], "objective", repr(plain["objective"]),
          repr(res["objective"]), "error", plain["error"], res["error"])
    assert plain["failed"] == 0 and plain["status"] == mref.CONVERGED and plain["error"] <= 1e-8
    assert res["failed"] == 0 and res["status"] == mref.CONVERGED and res["error"] <= 1e-8
    assert abs(res["objective"] - plain["objective"]) <= 1e-6
