"""The quality-function oracle's arithmetic and refusals without a GPU: tests/qf_reference.py (the numpy restatement of
csrc/iem_qf_device.h) against tests/amu_reference.py, tests/mu_reference.py and tests/barrier_reference.py.

(a) symbols, struct sizes, the defaults stated twice, the refusals that need no device;
(b) the source: a code object of its own behind the helpers, the integer minimum its only atomic call, no scratch;
(c) the combination d0 + t·(d1 − d0) is the Newton direction at mu = sigma·avg;
(d) the section: the bracket of a convex quadratic, the least evaluated q on the five models, every branch of the state machine;
(e) the update: amu_reference.update of a LOQO object but for the oracle's words, mu_reference.update in fixed mode without progress."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import amu_reference as aref
import barrier_reference as bref
import mu_reference as mref
import qf_reference as qref

_HIPCC = "/opt/rocm/bin/hipcc"
CALLS = ("iem_qf_create", "iem_qf_destroy", "iem_qf_reset", "iem_qf_begin", "iem_qf_alpha", "iem_qf_value", "iem_qf_update", "iem_qf_device", "iem_qf_state",
         "iem_qf_source")
KERNELS = ("qf_alpha", "qf_begin", "qf_reset", "qf_update", "qf_value")
MODELS = ["opf_7", "pandemic_20x3", "farmer_5", "quadrotor_100", "test_problem_1"]      # the five of tests/test_barrier.py
N_WG = 2
# (c): the largest normalised difference measured on the CPU this was written on (pandemic_20x3, sigma = 50), and the bound: 4 x that
MEASURED_COMBINATION = 9.182e-12
BOUND_COMBINATION = 4.0 * MEASURED_COMBINATION


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


def word_vector(P, st):
    """the twelve words with the sums in numpy's order (any one order serves the CPU tests)"""
    head, sums, w8, w10, p = mref.error_words(P["B"], st, P["r"], P["c"])
    return np.array([*head, *(float(np.sum(t)) for t in sums), w8, float(np.sum(p)), w10, 0.0])


def test_symbols_and_bindings(built):
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.barrier import QualityFunction
    L = iemlib.lib()
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "iem.h")).read()
    for name in CALLS:
        assert name in iemlib.SYMBOLS and getattr(L, name).argtypes is not None and re.search(r"\bint " + name + r"\(", header), name
    assert C.sizeof(iemlib.QfOpts) == 48 and C.sizeof(iemlib.QfState) == 28 * 8
    assert iemlib.QfOpts._fields_[0][0] == "struct_size" and iemlib.QfState._fields_[0][0] == "struct_size"
    o = iemlib.QfOpts.defaults()
    assert {k: getattr(o, k) for k in qref.OPTS} == qref.OPTS      # the defaults, stated twice
    assert qref.options()["sigma_max"] == aref.OPTS["sigma_max"] == 100.0      # sigma_max = 0: the iem_amu object's
    assert len(iemlib.QF_STATUS) == 4 and iemlib.QF_STATUS[qref.DONE] == "done" and iemlib.QF_STATUS[qref.UNUSABLE] == "unusable"
    for method in ("begin", "alpha", "value", "section", "update", "reset", "state", "device", "close", "__enter__", "__exit__"):
        assert callable(getattr(QualityFunction, method)), method
    with pytest.raises(TypeError):
        iemlib.QfOpts.defaults(kappa=0.5)
    # the section of the contract names the constants the restatement uses
    assert "0.6180339887498949" in header and str(qref.GOLDEN) == "0.6180339887498949"


def test_the_source(built):
    """a code object of its own behind the helpers, compiled without contraction: the same text and key twice, the key fnv1a64 of the
    text and no other object's, its own five kernels only, the integer minimum as the only atomic call of its own text, no inline
    assembly and no pow of its own; no other object's source knows of it and the fixed sources are the three they were"""
    from infiniteexamodels.jl_amd import lib as iemlib
    src, key = iemlib.qf_source()
    assert iemlib.qf_source() == (src, key)
    h = 1469598103934665603
    for byte in src.encode():
        h = ((h ^ byte) * 1099511628211) & (2 ** 64 - 1)
    assert key == h
    fixed = list(iemlib.fixed_sources())
    assert len(fixed) == 3
    others = [k for _, _, k in fixed] + [f()[1] for f in (iemlib.search_source, iemlib.soc_source, iemlib.resto_source, iemlib.mu_source, iemlib.barrier_mu_source,
                                                          iemlib.amu_source)]
    assert key not in others and len(set(others)) == len(others)
    head = src.split("\n", 1)[0]
    assert head.startswith("// iem-flags:") and "-ffp-contract=off" in head
    prefix, own = src.split("// iem_qf_device.h", 1)
    assert "#define IEM_TILE 256" in prefix and "iem_shared_park" in prefix
    kernels = re.findall(r"__global__ [^\n]*void (\w+)\(", own)
    assert tuple(sorted(kernels)) == KERNELS and src.count("__global__") == len(KERNELS)
    code = "\n".join(line.split("//", 1)[0] for line in own.splitlines())
    assert re.findall(r"\batomic\w*\(", code) == ["atomicMin("]      # ONE call site: at most one atomic per workgroup and slot
    assert re.findall(r"__hip_atomic\w*", code) == ["__hip_atomic_load"]      # the relaxed look at the slot in front of it
    assert "asm" not in code and "pow(" not in code and "cooperative" not in code and "grid.sync" not in code
    for helper in ("iem_shared_park<", "iem_shared_last(", "iem_shared_totals("):
        assert helper in code, helper
    assert "iem_grad_atomic(" not in code and "iem_grad_wave_uniform(" not in code and "iem_last_arrival" not in code      # the helpers' float atomics stay unused
    assert len(re.findall(r"\bqf_dir\(", code)) > 12 and code.count("double qf_dir(") == 1      # ONE function forms the direction for both grid kernels
    # no other object's source knows of it
    for f in (iemlib.mu_source, iemlib.barrier_mu_source, iemlib.barrier_source, iemlib.search_source, iemlib.soc_source, iemlib.resto_source, iemlib.amu_source):
        assert "qf_" not in f()[0]
    assert all("qf_" not in text for _, text, _ in fixed)
    # the adaptive object keeps its three kernels
    assert iemlib.amu_source()[0].split("// iem_amu_device.h", 1)[1].count("__global__") == 3


@pytest.mark.skipif(not os.path.exists(_HIPCC), reason="no hipcc")
def test_the_object_compiles_without_scratch(built, tmp_path):
    from infiniteexamodels.jl_amd import lib as iemlib
    src, _ = iemlib.qf_source()
    head = src.split("\n", 1)[0]
    hip = tmp_path / "q.hip"
    hip.write_text(src)
    p = subprocess.run([_HIPCC, "--genco", "--offload-arch=gfx950", *head[len("// iem-flags:"):].split(), "-Rpass-analysis=kernel-resource-usage",
                        "-o", str(tmp_path / "q.hsaco"), str(hip)], capture_output=True, text=True)
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
    assert L.iem_qf_create(N, N, C.byref(out)) == -4 and "null" in err()
    assert L.iem_qf_create(N, C.byref(iemlib.QfOpts.defaults()), N) == -4 and "null" in err()
    assert L.iem_qf_destroy(N) == 0
    assert L.iem_qf_reset(N) == -4 and "null" in err()
    assert L.iem_qf_begin(N, *[N] * 10) == -4 and "null" in err()
    assert L.iem_qf_alpha(N, *[N] * 18) == -4 and "null" in err()
    assert L.iem_qf_value(N, *[N] * 18) == -4 and "null" in err()
    assert L.iem_qf_update(N, N, 0, N) == -4 and "null" in err()
    assert L.iem_qf_device(N, N) == -4 and "null" in err()
    assert L.iem_qf_state(N, N, N, N) == -4 and "null" in err()
    # iem_amu_create keeps refusing the oracle it does not have
    o = iemlib.AmuOpts.defaults(oracle=2)
    assert L.iem_amu_create(N, C.byref(o), C.byref(out)) == -4


# ---- (c) the combination -------------------------------------------------------------------------------------------------------------
def _avg(P):
    nz = P["B"]["counts"]["nz"]
    return float(np.sum(mref.products(P["B"], P["state"]))) / nz if nz else 1.0


@pytest.mark.parametrize("name", MODELS)
def test_the_combination_is_a_newton_direction(name, built):
    """d(sigma) = d0 + t·(d1 − d0), t = (sigma·avg)/mu_ref, against the direction computed DIRECTLY at mu = sigma·avg through the same
    restated formulas (terms, the LU of the host's KKT matrix, step), sigma in {1e-3, 1, 50}, every component the oracle reads on
    the entries it reads, the difference normalised by max(1, the largest entry of the direct direction).  Measured on the CPU
    this was written on: at most 9.182e-12 (pandemic_20x3, sigma = 50; opf_7 2.6e-12, farmer_5 6.2e-13, test_problem_1 5.9e-14,
    quadrotor_100 — no bound, the direction does not depend on mu — 0).  The bound is 4 x the measured value: 3.673e-11."""
    P = bref.barrier_point(name)
    B, st = P["B"], P["state"]
    avg = _avg(P)
    sigmas = (1e-3, 1.0, 50.0)
    d0, d1, direct = qref.two_columns(P, mus=[s * avg for s in sigmas])
    reads = [np.r_[np.ones(len(st[0]), dtype=bool), np.zeros(len(st[1]), dtype=bool)], ~B["eq"], B["hasL"], B["hasU"], B["gL"], B["gU"]]
    for sigma, want in zip(sigmas, direct):
        qb = qref.fresh_block()
        qb[qref.SIGMA], qb[qref.AVG] = sigma, avg
        got = qref.direction(d0, d1, qref.scale(qb, qref.options()))
        norm = max([1.0] + [float(np.abs(b[m]).max()) for b, m in zip(want, reads) if m.any()])
        diff = max([0.0] + [float(np.abs(a[m] - b[m]).max()) for a, b, m in zip(got, want, reads) if m.any()])
        print(name, "sigma", sigma, "avg", avg, "norm", norm, "difference / norm", diff / norm, "bound", BOUND_COMBINATION)
        assert diff / norm <= BOUND_COMBINATION
    # d1 = d0: the direction is d0 bit for bit
    same = qref.direction(d0, d0, np.float64(0.37))
    assert all(np.array_equal(bits(a[m] + 0.0), bits(b[m] + 0.0)) for a, b, m in zip(same, d0, reads))


# ---- (d) the section -----------------------------------------------------------------------------------------------------------------
def quadratic(k):
    """Two variables on lower bounds 0 with x = z = 1 (avg = 1, so t = sigma), dx = 0 and dzL(sigma) = (−0.5 + k·sigma, 2 − k·sigma):
    while k·sigma <= 2.99 both step lengths are 1, D2 = 0, and q(sigma) = ((0.5 + k·sigma)² + (3 − k·sigma)²)/2 — strictly convex with
    its minimiser at sigma = 1.25/k"""
    e, off = np.zeros(0), np.zeros(2, dtype=bool)
    B = dict(xl=np.zeros(2), xu=np.full(2, np.inf), rl=e, ru=e, ceq=e, eq=e.astype(bool), hasL=~off, hasU=off, gL=e.astype(bool), gU=e.astype(bool),
             counts=dict(nvar=2, ncon=0, n_eq=0, n_ineq=0, n_xl=2, n_xu=0, n_sl=0, n_su=0, nz=2))
    st = (np.ones(2), e, e, np.ones(2), np.full(2, np.nan), e, e)
    z2 = np.zeros(2)
    d0 = (z2, e, np.array([-0.5, 2.0]), z2, e, e)
    d1 = (z2, e, np.array([-0.5 + k, 2.0 - k]), z2, e, e)
    w = np.zeros(12)
    w[9] = 2.0
    return B, st, np.ones(2), e, w, d0, d1


def run(B, st, r, c, w, d0, d1, ab=None, aopts=None, trace=None, **over):
    aopts = aopts if aopts is not None else aref.options()
    qopts = qref.options(aopts, **over)
    qb = qref.begin(B, st, r, c, w, ab if ab is not None else aref.fresh_block(aopts), aopts, qopts, N_WG)
    first = qb.copy()
    return first, qref.section(B, st, d0, d1, qb, mref.fresh_block(mref.options()), qopts, N_WG, trace=trace), qopts


@pytest.mark.parametrize("k,sigma_max,half", [(2.5, 1.0, "left"), (0.25, 10.0, "right")])
@pytest.mark.parametrize("steps", [1, 8, 16])
def test_the_section_brackets_the_minimiser_of_a_quadratic(k, sigma_max, half, steps, built):
    """the result and the minimiser both lie in the final bracket, whose width is (b − a)·g^steps of the first one: no margin"""
    B, st, r, c, w, d0, d1 = quadratic(k)
    trace = []
    first, qb, qopts = run(B, st, r, c, w, d0, d1, trace=trace, sigma_max=sigma_max, max_section_steps=steps, section_sigma_tol=1e-9)
    want = 1.25 / k
    assert bits(first[qref.D2]) == bits(0.0) and first[qref.AVG] == 1.0 and (first[qref.LO], first[qref.HI], first[qref.SIGMA]) == (1e-6, sigma_max, 1.0)
    assert qref.ints(qb)[qref.STATUS] == qref.DONE and qref.ints(qb)[qref.STEPS] == steps and qref.ints(qb)[qref.EVALS] == steps + 4 == len(trace)
    for sigma, q, blk in trace:      # the closed form, where both step lengths are 1
        assert (blk[qref.LAST_AP], blk[qref.LAST_AD]) == (1.0, 1.0)
        assert np.isclose(q, ((0.5 + k * sigma) ** 2 + (3.0 - k * sigma) ** 2) / 2.0, rtol=1e-14, atol=0.0)
    a0, b0 = (1e-6, trace[1][0]) if half == "left" else (1.0, sigma_max)
    assert (trace[1][1] <= trace[0][1]) == (half == "left") and trace[1][0] == 1.0 * (1.0 - 1e-2)
    a, b = qb[qref.A_], qb[qref.B_]
    width = (b0 - a0) * qref.GOLDEN ** steps
    print(half, "steps", steps, "bracket", a, b, "width", b - a, "derived", width, "result", qb[qref.BEST], "minimiser", want)
    assert np.isclose(b - a, width, rtol=1e-12, atol=0.0)
    assert a <= want <= b and a <= qb[qref.BEST] <= b and abs(qb[qref.BEST] - want) <= width
    assert qb[qref.QBEST] == min(q for _, q, _ in trace)


@pytest.mark.parametrize("name", MODELS)
def test_the_section_returns_the_least_evaluated_value(name, built):
    """on the five models: the result's q is <= every evaluated q and <= q(first sigma); the first of equal values wins; the pairs
    behind the end change nothing"""
    P = bref.barrier_point(name)
    B, st = P["B"], P["state"]
    d0, d1, _ = qref.two_columns(P)
    trace = []
    first, qb, qopts = run(B, st, P["r"], P["c"], word_vector(P, st), d0, d1, trace=trace)
    iq = qref.ints(qb)
    if B["counts"]["nz"] == 0:
        assert iq[qref.STATUS] == qref.DONE and trace == [] and iq[qref.EVALS] == 0 and bits(qb[qref.SIGMA]) == bits(0.0)      # nz == 0: straight to DONE
        assert qb[qref.D2] > 0.0 and qb[qref.P2] > 0.0
        return
    print(name, "lo", qb[qref.LO], "hi", qb[qref.HI], "evaluations", [(s, q) for s, q, _ in trace], "result", qb[qref.BEST], qb[qref.QBEST])
    assert iq[qref.STATUS] == qref.DONE and 2 <= len(trace) == iq[qref.EVALS] <= qopts["max_section_steps"] + 4
    qs = [q for _, q, _ in trace]
    assert qb[qref.QBEST] == min(qs) and qb[qref.QBEST] <= qs[0] == qb[qref.Q0] and np.isfinite(qs).all()
    assert qb[qref.BEST] == trace[qs.index(min(qs))][0]      # list.index: the first of equal values
    assert all(qb[qref.LO] <= s <= qb[qref.HI] for s, _, _ in trace) and trace[0][0] == first[qref.SIGMA]
    again = qref.section(B, st, d0, d1, qb, mref.fresh_block(mref.options()), qopts, N_WG, pairs=3)
    assert np.array_equal(bits(again), bits(qb))


def test_every_branch_of_the_section(built):
    B, st, r, c, w, d0, d1 = quadratic(0.25)
    status = lambda qb: int(qref.ints(qb)[qref.STATUS])
    # stop by the step count (the default tolerance is never met on [1, 10] in 8 steps), and early by the tolerance
    _, qb, _ = run(B, st, r, c, w, d0, d1, sigma_max=10.0)
    assert status(qb) == qref.DONE and qref.ints(qb)[qref.STEPS] == 8 and qref.ints(qb)[qref.EVALS] == 12 and qb[qref.B_] - qb[qref.A_] > 1e-2 * qb[qref.B_]
    _, qb, _ = run(B, st, r, c, w, d0, d1, sigma_max=10.0, section_sigma_tol=0.2, max_section_steps=16)
    assert status(qb) == qref.DONE and 0 < qref.ints(qb)[qref.STEPS] < 16 and qb[qref.B_] - qb[qref.A_] <= 0.2 * qb[qref.B_]
    assert qref.ints(qb)[qref.EVALS] == qref.ints(qb)[qref.STEPS] + 3      # the point of the step that met the tolerance is not evaluated
    # the first bracket already within the tolerance: two evaluations
    _, qb, _ = run(B, st, r, c, w, d0, d1, sigma_max=10.0, section_sigma_tol=0.95)
    assert status(qb) == qref.DONE and qref.ints(qb)[qref.EVALS] == 2 and qref.ints(qb)[qref.PHASE] == qref.SECOND
    # lo == hi
    first, qb, _ = run(B, st, r, c, w, d0, d1, sigma_min=2.0, sigma_max=2.0)
    assert first[qref.LO] == first[qref.HI] == first[qref.SIGMA] == 2.0
    assert status(qb) == qref.DONE and qref.ints(qb)[qref.EVALS] == 2 and qb[qref.BEST] == 2.0 and qb[qref.A_] == qb[qref.B_] == 2.0
    # the bracket of sigma clamped at mu_min (lo = mu_min/avg) and at mu_max (hi = mu_max/avg: word 1 of the iem_amu block, or mu_max_fact·avg)
    ao = aref.options(mu_min=0.5)
    first, qb, _ = run(B, st, r, c, w, d0, d1, aopts=ao, sigma_max=10.0)
    assert first[qref.LO] == 0.5 and first[qref.SIGMA] == 1.0 and status(qb) == qref.DONE and qb[qref.BEST] >= 0.5
    first, qb, _ = run(B, st, r, c, w, d0, d1, ab=aref.own_block(aref.options(), mu_max=4.0))
    assert first[qref.HI] == 4.0 and status(qb) == qref.DONE and qb[qref.BEST] <= 4.0
    first, _, _ = run(B, st, r, c, w, d0, d1, aopts=aref.options(mu_max_fact=3.0))
    assert first[qref.HI] == 3.0
    first, _, _ = run(B, st, r, c, w, d0, d1, aopts=aref.options(mu_min=5.0), sigma_max=10.0)
    assert first[qref.LO] == 5.0 and first[qref.SIGMA] == 5.0      # the first trial is min(max(1, lo), hi)
    first, _, _ = run(B, st, r, c, w, d0, d1, sigma_max=0.5)
    assert first[qref.HI] == 0.5 and first[qref.SIGMA] == 0.5
    # every evaluation +inf: a NaN in a direction at a present bound (alpha_dual = +0.0), a NaN product, a step length of +0.0
    bad = (d1[0], d1[1], np.array([np.nan, 1.0]), d1[3], d1[4], d1[5])
    trace = []
    _, qb, _ = run(B, st, r, c, w, d0, bad, trace=trace, sigma_max=10.0)
    assert status(qb) == qref.UNUSABLE and len(trace) == 12 and all(np.isposinf(q) for _, q, _ in trace) and qb[qref.BEST] == 1.0
    assert all(blk[qref.LAST_AD] == 0.0 for _, _, blk in trace)
    q = qref.fresh_block()
    assert np.isposinf(qref.quality(q, 1.0, 1.0, 1.0, 1.0, (2, 0, 2))) and np.isposinf(qref.quality(q, 1.0, 0.0, 0.0, 1.0, (2, 0, 2)))
    assert np.isposinf(qref.quality(q, np.nan, 0.0, 1.0, 1.0, (2, 0, 2))) and qref.quality(q, 3.0, 0.0, 1.0, 1.0, (2, 0, 2)) == 1.5
    q[qref.D2], q[qref.P2] = 8.0, 6.0
    assert qref.quality(q, 2.0, 0.0, 0.5, 0.75, (4, 3, 2)) == (0.0625 * 8.0) / 4 + (0.25 * 6.0) / 3 + 1.0      # a term whose count is 0 is +0.0: above
    # an idle, a finished and an unusable section: alpha and value change nothing
    for blk in (qref.fresh_block(), qb, qref.done_block(0.3)):
        assert np.array_equal(bits(qref.alpha(B, st, d0, d1, blk, mref.fresh_block(mref.options()), qref.options())), bits(blk))
        assert np.array_equal(bits(qref.value(B, st, d0, d1, blk, qref.options(), N_WG)), bits(blk))


def test_the_sums_have_the_order_of_the_grid(built):
    """device_sum: one workgroup of one lane is the plain loop; any grid lies within the bound of a summation order; D2 and P2 of
    `begin` are sums of the squares of barrier_reference.error's residuals"""
    rng = np.random.default_rng(5)
    a = rng.standard_normal(3000) ** 2
    loop = np.float64(0.0)
    for v in a[:1]:
        loop = loop + v
    assert bits(qref.device_sum([a[:1]], 1)) == bits(loop)
    fs, bound = bref.sum_bound(a)
    for n_wg in (1, 2, 5, 70):
        assert abs(qref.device_sum([a], n_wg) - fs) <= bound
    assert bits(qref.device_sum([a, a], 3)) != bits(qref.device_sum([a], 3))
    P = bref.barrier_point("opf_7")
    B, st = P["B"], P["state"]
    qb = qref.begin(B, st, P["r"], P["c"], word_vector(P, st), aref.fresh_block(aref.options()), aref.options(), qref.options(), N_WG)
    x, s, y, zL, zU, vL, vU = st
    z = lambda v, on: np.where(on, v, 0.0)
    t = P["r"] - z(zL, B["hasL"]) + z(zU, B["hasU"])
    u = (-y - z(vL, B["gL"]) + z(vU, B["gU"]))[~B["eq"]]
    inf = np.where(B["eq"], P["c"] - B["ceq"], P["c"] - s)
    assert np.isclose(qb[qref.D2], np.sum(t * t) + np.sum(u * u), rtol=1e-12) and np.isclose(qb[qref.P2], np.sum(inf * inf), rtol=1e-12)


# ---- (e) the update ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counts", [(31, 17), (0, 5), (4, 0)])
def test_the_update_is_the_adaptive_rule(counts, built):
    """with the same w12, blocks and options qf_reference.update equals amu_reference.update of a LOQO object bit for bit in every
    word except words 7, 8, 10 of the iem_amu block and, in free mode, mu, tau, zeta — and word 4 of the iem_mu block, which is E AT
    the mu the call leaves: it is checked against E of the restatement at that mu, and the flag against the change of mu's bits"""
    aopts = aref.options(oracle=aref.LOQO)
    seen = set()
    for case in aref.branch_cases(aref.LOQO, counts):
        ctl = np.arange(16, dtype=np.float64) + 1.0
        for sigma in (0.3, 1e-14, 1e6):      # unclamped, clamped at mu_min, clamped at mu_max
            qb = qref.done_block(sigma, 2.5)
            ref, ab_ref, ctl_ref = aref.update(case["blk"], case["ab"], case["w"], None, counts, case["opts"], case["aopts"], case["force_fixed"], ctl)
            got, ab, ctl2 = qref.update(case["blk"], case["ab"], qb, case["w"], counts, case["opts"], case["aopts"], case["force_fixed"], ctl)
            iw, ia = mref.ints(got), mref.ints(ab)
            free = iw[8] == mref.ITERATING and counts[1] != 0 and ia[aref.MODE] == aref.FREE
            own = [i for i in range(16) if i not in (aref.MU_ORACLE, aref.SIGMA, aref.M_AFF)]
            assert bits(ab[own]).tolist() == bits(ab_ref[own]).tolist(), case["label"]
            if free:
                avg = ab[aref.AVG]
                assert bits(ab[aref.SIGMA]) == bits(sigma) and bits(ab[aref.MU_ORACLE]) == bits(np.float64(sigma) * avg) and ab[aref.M_AFF] == 2.5
                mu = np.minimum(np.maximum(np.float64(sigma) * avg, np.float64(case["aopts"]["mu_min"])), ab[aref.MU_MAX])
                assert bits(got[0]) == bits(mu), case["label"]
                seen.add("mu_min" if mu == case["aopts"]["mu_min"] else "mu_max" if mu == ab[aref.MU_MAX] else "unclamped")
                changed = bits(mu) != bits(case["blk"][0])
                assert bool(iw[9] & 1) == changed and (bits(ctl2[11:13]).tolist() == [0, 0]) == changed
                if changed:
                    assert bits(got[1]) == bits(np.maximum(np.float64(case["opts"]["tau_min"]), 1.0 - mu)) and bits(got[2]) == bits(np.sqrt(mu))
                assert bits(got[4]) == bits(mref.E(case["w"], counts, case["opts"], got[0]))
                rest = [3, 5, 6, 7, 8, 10, 11, 12, 13, 14, 15]
                assert bits(got[rest]).tolist() == bits(ref[rest]).tolist(), case["label"]
            else:
                assert bits(got).tolist() == bits(ref).tolist() and bits(ctl2).tolist() == bits(ctl_ref).tolist(), case["label"]
                assert bits(ab).tolist() == bits(ab_ref).tolist(), case["label"]      # the oracle's words stay
        # a section that is not DONE: UNUSABLE, mu and the iem_amu block stay
        for blk in (qref.fresh_block(), qref.done_block(0.3)):
            qref.ints(blk)[qref.STATUS] = qref.IDLE if blk[qref.BEST] == 0.0 else qref.UNUSABLE
            got, ab, ctl2 = qref.update(case["blk"], case["ab"], blk, case["w"], counts, case["opts"], case["aopts"], case["force_fixed"], ctl)
            assert mref.ints(got)[8] == mref.UNUSABLE and bits(got[:3]).tolist() == bits(case["blk"][:3]).tolist() and bits(ab).tolist() == bits(case["ab"]).tolist()
            assert bits(ctl2).tolist() == bits(ctl).tolist() and mref.ints(got)[11] == 1 and not mref.ints(got)[9] & 1
    assert seen == ({"unclamped", "mu_min", "mu_max"} if counts[1] else set())


@pytest.mark.parametrize("name", ["opf_7", "pandemic_20x3"])
def test_fixed_mode_without_progress_is_the_monotone_rule(name, built):
    aopts = aref.options()
    for label, P, st, blk, opts, want in mref.branch_cases(name):
        counts = (P["B"]["counts"]["ncon"], P["B"]["counts"]["nz"])
        w = word_vector(P, st)
        ctl = np.arange(16, dtype=np.float64) + 1.0
        ab = aref.own_block(aopts, aref.FIXED, 1e300, (0.0,) * 4)      # no E(0) > 0 is progress against references of zero
        ref, ctl_ref = mref.update(blk, w, counts, opts, ctl)
        got, ab2, ctl2 = qref.update(blk, ab, qref.done_block(0.3), w, counts, opts, aopts, False, ctl)
        assert bits(got).tolist() == bits(ref).tolist(), (label, got, ref)      # mu, tau, zeta, the errors, status, flag, decreases, updates
        assert bits(ctl2).tolist() == bits(ctl_ref).tolist()
        assert mref.ints(ab2)[aref.MODE] == aref.FIXED and mref.ints(ab2)[aref.TO_FREE] == 0


@pytest.mark.parametrize("name,want,iterations", [("rosenbrock", 306.4999755050365, 25), ("ode_5x5", -12.784599900757165, 7)])
def test_the_restated_rule_converges_on_the_host(name, want, iterations, built):
    """qf_reference.host_loop — tests/qf_loop.py made of the restatements alone, a dense solve in the place of the solver object —
    reaches the optima the device loops are held to, to their tolerance, without a failed search.  The iteration counts of this
    host (25 and 7) are printed beside what was found, not asserted: the solves differ from the device's in the last bits."""
    import cases
    from infiniteexamodels.jl_amd import transcribe
    from pyoracle import OracleModel
    core = transcribe.exa_core(cases.rosenbrock()[0]) if name == "rosenbrock" else cases.build_core(name)
    res = qref.host_loop(OracleModel(core.to_blob()))
    print(name, "iterations", res["iterations"], "(written with", iterations, ") objective", repr(res["objective"]), "error", res["error"], "to_fixed", res["to_fixed"],
          "to_free", res["to_free"], "mu", ["%.3e" % v for v in res["mus"]], "sigma", ["%.3g" % v for v in res["sigmas"]])
    assert res["failed"] == 0 and res["status"] == mref.CONVERGED and res["error"] <= 1e-8 and abs(res["objective"] - want) <= 1e-6
