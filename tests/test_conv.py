"""The stopping test's arithmetic and refusals without a GPU: tests/conv_reference.py (the numpy restatement of
csrc/iem_conv_device.h) against tests/mu_reference.py and against the contract of include/iem.h.

(a) symbols, struct sizes, the defaults stated twice, the refusals that need no device;
(b) the source: a code object of its own behind the helpers, the integer maximum its only atomic call, no scratch;
(c) E(0) is word 3 of mu_reference.update on random twelve-word inputs, bit for bit;
(d) every branch of the decision in the stated order, every tolerance at its value and at the next double above, the latch;
(e) the tiny-step branches and flags;
(f) keep and restore on every kind of bound, the maxima on bit patterns."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import barrier_reference as bref
import conv_reference as cref
import mu_reference as mref

_HIPCC = "/opt/rocm/bin/hipcc"
CALLS = ("iem_conv_create", "iem_conv_destroy", "iem_conv_reset", "iem_conv_check", "iem_conv_keep", "iem_conv_restore", "iem_conv_step", "iem_conv_kept",
         "iem_conv_device", "iem_conv_state", "iem_conv_source")
KERNELS = ("conv_decide", "conv_keep", "conv_reset", "conv_restore", "conv_step_decide", "conv_stepmax", "conv_xmax")
NAN, INF = float("nan"), float("inf")
up = lambda v: float(np.nextafter(v, INF))


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def test_symbols_and_bindings(built):
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.barrier import ConvergenceCheck
    L = iemlib.lib()
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "iem.h")).read()
    for name in CALLS:
        assert name in iemlib.SYMBOLS and getattr(L, name).argtypes is not None and re.search(r"\bint " + name + r"\(", header), name
    assert C.sizeof(iemlib.ConvOpts) == 14 * 8 and C.sizeof(iemlib.ConvState) == 20 * 8
    assert iemlib.ConvOpts._fields_[0][0] == "struct_size" and iemlib.ConvState._fields_[0][0] == "struct_size"
    o = iemlib.ConvOpts.defaults()
    assert {k: getattr(o, k) for k in cref.OPTS} == cref.OPTS == iemlib.ConvOpts.DEFAULTS      # the defaults, stated twice
    assert cref.OPTS["tiny_step_tol"] == 10.0 * np.finfo(np.float64).eps and cref.OPTS["max_iter"] == 3000 and cref.OPTS["acceptable_iter"] == 15
    for method in ("check", "keep", "restore", "step", "kept", "reset", "state", "device", "close", "__enter__", "__exit__"):
        assert callable(getattr(ConvergenceCheck, method)), method
    with pytest.raises(TypeError):
        iemlib.ConvOpts.defaults(tol=1e-8)      # tol is the iem_mu object's
    assert iemlib.CONV_STATUS == ("iterating", "converged", "acceptable", "maxiter", "diverging", "invalid", "tiny_step")
    assert [f for f, _ in iemlib.ConvState._fields_[1:]] == ["status", "checks", "acceptable_count", "keep", "kept", "kept_at", "flags", "tiny_count", "e0", "dual_inf",
                                                            "constr_viol", "compl_inf", "f", "f_prev", "xmax", "kept_e0", "kept_f", "rel", "dymax"]


def test_the_source(built):
    """a code object of its own behind the helpers, compiled without contraction: the same text and key twice, the key fnv1a64 of the
    text and no other object's, its own seven kernels, the integer maximum as the only atomic call of its own text, no inline
    assembly; no other object's source knows of it and the fixed sources are the three they were"""
    from infiniteexamodels.jl_amd import lib as iemlib
    src, key = iemlib.conv_source()
    assert iemlib.conv_source() == (src, key)
    h = 1469598103934665603
    for byte in src.encode():
        h = ((h ^ byte) * 1099511628211) & (2 ** 64 - 1)
    assert key == h
    fixed = list(iemlib.fixed_sources())
    assert len(fixed) == 3
    siblings = (iemlib.search_source, iemlib.soc_source, iemlib.resto_source, iemlib.mu_source, iemlib.barrier_mu_source, iemlib.amu_source, iemlib.qf_source,
                iemlib.mpc_source, iemlib.init_source)
    others = [k for _, _, k in fixed] + [f()[1] for f in siblings]
    assert key not in others and len(set(others)) == len(others)
    assert all(text != src for _, text, _ in fixed)
    head = src.split("\n", 1)[0]
    assert head.startswith("// iem-flags:") and "-ffp-contract=off" in head
    prefix, own = src.split("// iem_conv_device.h", 1)
    assert "#define IEM_TILE 256" in prefix
    kernels = re.findall(r"__global__ [^\n]*void (\w+)\(", own)
    assert tuple(sorted(kernels)) == KERNELS and src.count("__global__") == len(KERNELS)
    code = "\n".join(line.split("//", 1)[0] for line in own.splitlines())
    assert re.findall(r"\batomic\w*\(", code) == ["atomicMax("]      # ONE call site, on 64-bit integers: no atomicAdd on a float
    assert re.findall(r"__hip_atomic\w*", code) == ["__hip_atomic_load"]      # the relaxed look at the slot in front of it
    assert "atomicAdd" not in code and "asm" not in code and "cooperative" not in code and "grid.sync" not in code
    assert "iem_grad_atomic(" not in code and "iem_grad_wave_uniform(" not in code      # the helpers' float atomics stay unused
    for f in siblings + (iemlib.barrier_source,):
        assert "conv_decide" not in f()[0] and "conv_keep" not in f()[0]
    assert all("conv_decide" not in text for _, text, _ in fixed)


@pytest.mark.skipif(not os.path.exists(_HIPCC), reason="no hipcc")
def test_the_object_compiles_without_scratch(built, tmp_path):
    from infiniteexamodels.jl_amd import lib as iemlib
    src, _ = iemlib.conv_source()
    head = src.split("\n", 1)[0]
    hip = tmp_path / "c.hip"
    hip.write_text(src)
    p = subprocess.run([_HIPCC, "--genco", "--offload-arch=gfx950", *head[len("// iem-flags:"):].split(), "-Rpass-analysis=kernel-resource-usage",
                        "-o", str(tmp_path / "c.hsaco"), str(hip)], capture_output=True, text=True)
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
    assert L.iem_conv_create(N, N, C.byref(out)) == -4 and "null" in err()
    assert L.iem_conv_create(N, C.byref(iemlib.ConvOpts.defaults()), N) == -4 and "null" in err()
    assert L.iem_conv_destroy(N) == 0
    assert L.iem_conv_reset(N) == -4 and "null" in err()
    assert L.iem_conv_check(N, N, N, N) == -4 and "null" in err()
    assert L.iem_conv_keep(N, *[N] * 7) == -4 and "null" in err()
    assert L.iem_conv_restore(N, *[N] * 7) == -4 and "null" in err()
    assert L.iem_conv_step(N, N, N, N, N) == -4 and "null" in err()
    assert L.iem_conv_kept(N, *[N] * 7) == -4 and "null" in err()
    assert L.iem_conv_device(N, N) == -4 and "null" in err()
    assert L.iem_conv_state(N, N) == -4 and "null" in err()


# ---- (c) E(0) -----------------------------------------------------------------------------------------------------------------------------
def test_e0_is_word_3_of_mu_update(built):
    """on random twelve-word inputs — every count shape, zeros, infinities and NaN among the words — the restated E(0) carries the
    bits of word 3 of mu_reference.update, and d, p, cpl are the words the contract names"""
    rng = np.random.default_rng(7)
    seen_nan = 0
    for trial in range(400):
        w = np.exp(rng.uniform(-30, 10, 12)) * rng.choice([1.0, 1.0, 1.0, 0.0], 12)
        w[10] = 0.0
        if trial % 9 == 0:
            w[rng.integers(0, 9)] = rng.choice([NAN, INF])
        counts = [(5, 7), (0, 7), (5, 0), (0, 0), (1, 1)][trial % 5]
        mo = mref.options(s_max=[100.0, 1.0, 3.7][trial % 3])
        blk, _ = mref.update(mref.fresh_block(mo), w, counts, mo)
        e0, d, p, cpl = cref.e0_terms(w, counts, mo)
        assert same(e0, blk[3]), (trial, w, counts)
        seen_nan += bool(np.isnan(e0))
        with np.errstate(invalid="ignore"):
            assert same(d, np.maximum(w[0], w[1])) and same(p, w[2] if counts[0] else 0.0) and same(cpl, w[3] if counts[1] else 0.0)
    assert seen_nan > 0


# ---- (d) the decision ---------------------------------------------------------------------------------------------------------------------
COUNTS = (3, 4)
MO = mref.options()      # tol 1e-8, s_max 100


def words(e=1.0, d=None, p=None, cpl=None, w10=0.0):
    """twelve words with sd = sc = 1 (w4 = w5 = 0) whose E(0) is max(d, p, cpl): each of the three set on its own; e: all three"""
    w = np.zeros(12)
    d, p, cpl = (e if v is None else v for v in (d, p, cpl))
    w[0], w[1], w[2], w[3], w[8], w[10] = d, 0.5 * d, p, cpl, 0.0, w10
    return w


def run(blk, w, f=1.0, x_max=1.0, counts=COUNTS, mo=MO, **over):
    return cref.decide(blk, w, f, x_max, counts, cref.options(**over), mo)


def facts(blk):
    iw = cref.ints(blk)
    return dict(status=int(iw[0]), checks=int(iw[1]), count=int(iw[2]), keep=int(iw[3]), kept=int(iw[4]), kept_at=int(iw[5]), flags=int(iw[6]))


def test_the_words_of_a_check(built):
    w = words(d=3.0, p=2.0, cpl=1.0)
    blk = run(cref.fresh_block(), w, f=-7.5, x_max=42.0)
    assert same(blk[8:15], [3.0, 3.0, 2.0, 1.0, -7.5, 0.0, 42.0]) and facts(blk) == dict(status=0, checks=1, count=0, keep=0, kept=0, kept_at=0, flags=0)
    assert not blk[15:].any()
    blk = run(blk, w, f=-8.0, x_max=43.0)
    assert same(blk[12:15], [-8.0, -7.5, 43.0]) and facts(blk)["checks"] == 2      # word 13: the f of the previous check
    # ncon = 0: p is +0.0 whatever word 2 holds; nz = 0: cpl is +0.0 and E(0) has no complementarity term
    blk = run(cref.fresh_block(), words(d=1e-9, p=5.0, cpl=1e-9), counts=(0, 4))
    assert same(blk[10], 0.0) and same(blk[8], 1e-9) and facts(blk)["status"] == cref.CONVERGED
    blk = run(cref.fresh_block(), words(d=1e-9, p=1e-9, cpl=5.0), counts=(3, 0))
    assert same(blk[11], 0.0) and same(blk[8], 1e-9) and facts(blk)["status"] == cref.CONVERGED
    blk = run(cref.fresh_block(), words(d=1e-9, p=NAN, cpl=NAN), counts=(0, 0))
    assert same(blk[8:12], [1e-9, 1e-9, 0.0, 0.0]) and facts(blk)["status"] == cref.CONVERGED


def test_branch_1_invalid(built):
    """w10 != 0; a NaN in E(0), f, xmax in turn; an infinity in E(0) and in f; an infinite xmax is NOT invalid (it diverges); INVALID
    comes first: the point below would converge"""
    good = words(1e-9)
    for label, kw in (("w10", dict(w=words(1e-9, w10=1.0))), ("w10 NaN", dict(w=words(1e-9, w10=NAN))), ("E0 NaN", dict(w=words(1e-9, d=NAN))), ("f NaN", dict(w=good, f=NAN)),
                      ("xmax NaN", dict(w=good, x_max=NAN)), ("E0 inf", dict(w=words(1e-9, p=INF))), ("f inf", dict(w=good, f=INF)), ("f -inf", dict(w=good, f=-INF))):
        blk = run(cref.fresh_block(), **kw)
        assert facts(blk) == dict(status=cref.INVALID, checks=0, count=0, keep=0, kept=0, kept_at=0, flags=0), label
    assert facts(run(cref.fresh_block(), good))["status"] == cref.CONVERGED
    assert facts(run(cref.fresh_block(), words(1.0), x_max=INF))["status"] == cref.DIVERGING
    # a held point survives an INVALID check; the acceptable flag is cleared
    blk = run(cref.fresh_block(), words(1e-7))
    assert facts(blk)["kept"] == 1 and facts(blk)["flags"] == 1
    bad = run(blk, words(1e-7), f=NAN)
    assert facts(bad) == dict(status=cref.INVALID, checks=1, count=1, keep=0, kept=1, kept_at=0, flags=0) and same(bad[15:17], blk[15:17])


def test_branch_2_converged(built):
    """each of the four tolerances at exactly its value and at the next double above; +inf tolerances; CONVERGED keeps the point"""
    tol = MO["tol"]
    off = dict(acceptable_tol=1e-30)      # nothing is acceptable: what misses branch 2 iterates
    at = dict(dual_inf_tol=1e-9, constr_viol_tol=2e-9, compl_inf_tol=3e-9)
    exact = words(d=1e-9, p=2e-9, cpl=3e-9)
    assert facts(run(cref.fresh_block(), exact, **at, **off)) == dict(status=cref.CONVERGED, checks=0, count=0, keep=1, kept=1, kept_at=0, flags=0)
    for k, (name, v) in enumerate((("d", 1e-9), ("p", 2e-9), ("cpl", 3e-9))):
        over = run(cref.fresh_block(), words(**{**dict(d=1e-9, p=2e-9, cpl=3e-9), name: up(v)}), **at, **off)
        assert facts(over)["status"] == cref.ITERATING and facts(over)["keep"] == 0, name
    assert facts(run(cref.fresh_block(), words(tol), **off))["status"] == cref.CONVERGED      # E(0) == tol exactly
    assert facts(run(cref.fresh_block(), words(up(tol)), **off))["status"] == cref.ITERATING
    # +inf switches the unscaled tests off; E(0) <= tol stays (sd = 1e3 scales d down: E(0) = 5e-9, d = 5e-6)
    w = words(d=5e-6, p=1e-9, cpl=1e-9)
    w[4] = 1e5 * sum(COUNTS)
    assert same(cref.e0_terms(w, COUNTS, MO)[0], 5e-6 / 1e3)
    assert facts(run(cref.fresh_block(), w, dual_inf_tol=1e-6, **off))["status"] == cref.ITERATING
    assert facts(run(cref.fresh_block(), w, dual_inf_tol=INF, constr_viol_tol=INF, compl_inf_tol=INF, **off))["status"] == cref.CONVERGED
    # a converged point replaces a kept acceptable one, whatever its E(0)
    blk = run(cref.fresh_block(), words(1e-7))
    blk = run(blk, words(1e-9), f=2.0)
    assert facts(blk) == dict(status=cref.CONVERGED, checks=1, count=1, keep=1, kept=1, kept_at=1, flags=0) and same(blk[15:17], [1e-9, 2.0])


def test_branch_3_acceptable(built):
    a = dict(acceptable_tol=1e-3, acceptable_dual_inf_tol=2e-3, acceptable_constr_viol_tol=3e-3, acceptable_compl_inf_tol=4e-3, acceptable_iter=3)
    # each acceptable tolerance at its value and at the next double above (E(0) = max of the three words here)
    assert facts(run(cref.fresh_block(), words(1e-3), **a))["flags"] == 1
    assert facts(run(cref.fresh_block(), words(up(1e-3)), **a))["flags"] == 0
    wide = dict(a, acceptable_tol=1.0)
    for name, v in (("d", 2e-3), ("p", 3e-3), ("cpl", 4e-3)):
        base = dict(d=1e-4, p=1e-4, cpl=1e-4)
        assert facts(run(cref.fresh_block(), words(**{**base, name: v}), **wide))["flags"] == 1, name
        assert facts(run(cref.fresh_block(), words(**{**base, name: up(v)}), **wide))["flags"] == 0, name
    # +inf acceptable tolerances: only E(0) <= acceptable_tol is left
    allinf = dict(acceptable_tol=1.0, acceptable_dual_inf_tol=INF, acceptable_constr_viol_tol=INF, acceptable_compl_inf_tol=INF, acceptable_obj_change_tol=INF)
    assert facts(run(cref.fresh_block(), words(0.5), **allinf))["flags"] == 1
    # the objective change: met at the first check whatever f; afterwards |f − f_prev| / max(1, |f|) at the tolerance and above
    oc = dict(a, acceptable_obj_change_tol=0.25)
    blk = run(cref.fresh_block(), words(1e-4), f=1e30, **oc)
    assert facts(blk) == dict(status=0, checks=1, count=1, keep=1, kept=1, kept_at=0, flags=1)
    blk = run(cref.fresh_block(), words(1e-4), f=8.0, **oc)
    assert facts(run(blk, words(1e-4), f=10.0, **oc))["flags"] == 1      # |10 − 8| / 10 = 0.2: the NEW f divides (2 / 8 would sit at the tolerance)
    assert facts(run(blk, words(1e-4), f=6.0, **oc))["flags"] == 0       # |6 − 8| / 6 > 0.25
    assert facts(run(blk, words(1e-4), f=-8.0, **oc))["flags"] == 0      # |−8 − 8| / 8 = 2
    f_at = 8.0 / 0.75      # f − 8 = 0.25 f up to rounding: decided by the rounded operations, checked against them
    diff, den = np.abs(np.float64(f_at) - np.float64(8.0)), np.maximum(np.float64(1.0), np.abs(np.float64(f_at)))
    assert facts(run(blk, words(1e-4), f=f_at, **oc))["flags"] == int(diff / den <= 0.25)
    small = run(cref.fresh_block(), words(1e-4), f=0.5, **oc)
    assert facts(run(small, words(1e-4), f=0.25, **oc))["flags"] == 1      # max(1, |f|) = 1: 0.25 / 1 at the tolerance
    assert facts(run(small, words(1e-4), f=up(0.75), **oc))["flags"] == 0
    # the count: grows, falls back to 0, ACCEPTABLE at acceptable_iter in a row
    blk = cref.fresh_block()
    trail = []
    for e in (1e-4, 1e-4, 5.0, 1e-4, 1e-4, 1e-4):
        blk = run(blk, words(e), **a)
        trail.append((facts(blk)["status"], facts(blk)["count"]))
    assert trail == [(0, 1), (0, 2), (0, 0), (0, 1), (0, 2), (cref.ACCEPTABLE, 3)] and facts(blk)["checks"] == 5
    # acceptable_iter = 0: no ACCEPTABLE stop, the points are still kept
    blk = cref.fresh_block()
    for k in range(20):
        blk = run(blk, words(1e-4), **dict(a, acceptable_iter=0))
    assert facts(blk) == dict(status=0, checks=20, count=20, keep=1, kept=1, kept_at=19, flags=1)
    # a better, an equal and a worse acceptable point after a kept one
    blk = run(cref.fresh_block(), words(1e-4), f=1.0, **a)
    worse = run(blk, words(2e-4), f=2.0, **a)
    assert facts(worse) == dict(status=0, checks=2, count=2, keep=0, kept=1, kept_at=0, flags=1) and same(worse[15:17], [1e-4, 1.0])
    equal = run(blk, words(1e-4), f=3.0, **a)
    assert facts(equal)["keep"] == 1 and facts(equal)["kept_at"] == 1 and same(equal[15:17], [1e-4, 3.0])
    better = run(worse, words(5e-5), f=4.0, **a)
    assert facts(better) == dict(status=cref.ACCEPTABLE, checks=2, count=3, keep=1, kept=1, kept_at=2, flags=1) and same(better[15:17], [5e-5, 4.0])
    # a point that is not acceptable never asks for a copy and leaves the kept words
    no = run(blk, words(5.0), **a)
    assert facts(no) == dict(status=0, checks=2, count=0, keep=0, kept=1, kept_at=0, flags=0) and same(no[15:17], blk[15:17])


def test_branches_4_and_5_and_the_order(built):
    # max_iter = 2: two checks pass, the third stops; max_iter = 0: the first check stops
    blk = cref.fresh_block()
    trail = []
    for _ in range(3):
        blk = run(blk, words(1.0), max_iter=2)
        trail.append((facts(blk)["status"], facts(blk)["checks"]))
    assert trail == [(0, 1), (0, 2), (cref.MAXITER, 2)]
    assert facts(run(cref.fresh_block(), words(1.0), max_iter=0))["status"] == cref.MAXITER
    # diverging: xmax at the tolerance and at the next double above
    assert facts(run(cref.fresh_block(), words(1.0), x_max=1e5, diverging_iterates_tol=1e5))["status"] == cref.ITERATING
    assert facts(run(cref.fresh_block(), words(1.0), x_max=up(1e5), diverging_iterates_tol=1e5))["status"] == cref.DIVERGING
    assert facts(run(cref.fresh_block(), words(1.0), x_max=INF, diverging_iterates_tol=INF))["status"] == cref.ITERATING
    # the order: CONVERGED before ACCEPTABLE before MAXITER before DIVERGING
    every = dict(max_iter=0, diverging_iterates_tol=1.0, acceptable_iter=1, acceptable_tol=1e-3)
    assert facts(run(cref.fresh_block(), words(1e-9), x_max=2.0, **every))["status"] == cref.CONVERGED
    acc = run(cref.fresh_block(), words(1e-4), x_max=2.0, **every)
    assert facts(acc)["status"] == cref.ACCEPTABLE and facts(acc)["keep"] == 1
    assert facts(run(cref.fresh_block(), words(1.0), x_max=2.0, **every))["status"] == cref.MAXITER
    assert facts(run(cref.fresh_block(), words(1.0), x_max=2.0, **dict(every, max_iter=1)))["status"] == cref.DIVERGING
    # an acceptable point at the MAXITER check is still kept
    m = run(cref.fresh_block(), words(1e-4), **dict(every, acceptable_iter=5))
    assert facts(m) == dict(status=cref.MAXITER, checks=0, count=1, keep=1, kept=1, kept_at=0, flags=1)


def test_the_latch(built):
    """behind every terminal status a check writes keep = 0 and nothing else, a step nothing; reset zeroes the block"""
    for first in (dict(w=words(1e-9)), dict(w=words(1e-7), acceptable_iter=1), dict(w=words(1.0), max_iter=0), dict(w=words(1.0), x_max=INF), dict(w=words(1.0), f=NAN)):
        w = first.pop("w")
        blk = run(cref.fresh_block(), w, **first)
        assert facts(blk)["status"] != 0
        again = run(blk, words(7.0), f=99.0, x_max=3.0, **{k: v for k, v in first.items() if k not in ("f", "x_max")})
        want = blk.copy()
        cref.ints(want)[cref.KEEP] = 0
        assert same(again, want)
        stepped = cref.step_decide(again, 0.0, 0.0, 0.0, cref.options(), MO)
        assert same(stepped, again)
    assert not cref.fresh_block().any() and len(cref.fresh_block()) == 24


# ---- (e) the tiny step --------------------------------------------------------------------------------------------------------------------
def test_the_tiny_step(built):
    o = cref.options()
    tol, ytol, floor = o["tiny_step_tol"], o["tiny_step_y_tol"], MO["mu_floor"]
    sd = lambda blk, rel, dy, mu: cref.step_decide(blk, rel, dy, mu, o, MO)
    f = lambda blk: (int(cref.ints(blk)[0]), int(cref.ints(blk)[6]), int(cref.ints(blk)[7]))
    below = float(np.nextafter(tol, 0.0))
    # rel at the tolerance is not tiny (strictly below is); a NaN compares false
    assert f(sd(cref.fresh_block(), tol, 0.0, floor)) == (0, 0, 0) and f(sd(cref.fresh_block(), NAN, 0.0, floor)) == (0, 0, 0)
    one = sd(cref.fresh_block(), below, 0.0, floor)
    assert f(one) == (0, 2, 1) and same(one[17:19], [below, 0.0])
    # the second tiny step in a row at the floor with a small dy: TINY_STEP
    two = sd(one, 0.0, 1e-3, floor)
    assert f(two) == (cref.TINY_STEP, 2, 2) and same(two[17:19], [0.0, 1e-3])
    # dymax at its tolerance is not small; mu above the floor: the hint, no stop; a NaN mu: neither
    assert f(sd(one, 0.0, ytol, floor)) == (0, 2, 2) and f(sd(one, 0.0, float(np.nextafter(ytol, 0.0)), floor))[0] == cref.TINY_STEP
    assert f(sd(one, 0.0, 0.0, up(floor))) == (0, 6, 2) and f(sd(one, 0.0, 0.0, NAN)) == (0, 2, 2) and f(sd(one, 0.0, NAN, floor)) == (0, 2, 2)
    # the count returns to 0 on a step that is not tiny and the flags clear; bit 0 (the check's) stays
    back = sd(sd(one, 0.0, 0.0, 1.0), 1.0, 5.0, 1.0)
    assert f(back) == (0, 0, 0) and same(back[17:19], [1.0, 5.0])
    blk = run(cref.fresh_block(), words(1e-7))
    assert f(blk)[1] == 1 and f(sd(blk, 0.0, 0.0, 1.0)) == (0, 7, 1)
    # and the check keeps bits 1 and 2
    assert f(run(sd(blk, 0.0, 0.0, 1.0), words(1.0)))[1] == 6
    # the maxima: rel over the variables and the inequality rows only, dymax over every row; a NaN wins
    B = bref.relaxed_bounds([0.0, -INF], [1.0, INF], [1.0, 0.0, -INF], [1.0, INF, 2.0], 0.0)
    x, s = np.array([3.0, -1.0]), np.array([NAN, 1.0, -3.0])
    sol, ds = np.array([2.0, -1.0, 9.0, -0.5, 0.25]), np.array([NAN, 1.0, -6.0])
    rel, dymax = cref.stepmax(B, x, s, sol, ds)
    assert same(rel, 6.0 / 4.0) and same(dymax, 9.0)      # the equality row's ds and s are never read, its dy is
    ds[1] = NAN
    assert np.isnan(cref.stepmax(B, x, s, sol, ds)[0]) and same(cref.stepmax(B, x, s, sol, ds)[1], 9.0)


# ---- (f) keep, restore, the maxima --------------------------------------------------------------------------------------------------------
def test_keep_and_restore(built):
    B = bref.relaxed_bounds([-INF, 1.0, -INF, 0.0], [INF, INF, 3.0, 10.0], [1.5, 0.0, -INF, -1.0], [1.5, INF, 2.0, 1.0], 0.0)
    assert B["eq"].tolist() == [True, False, False, False]
    st = (np.array([1.0, 2.0, 3.0, 4.0]), np.array([NAN, 5.0, 6.0, 7.0]), np.array([8.0, 9.0, 10.0, 11.0]), np.array([NAN, 12.0, NAN, 13.0]),
          np.array([NAN, NAN, 14.0, 15.0]), np.array([NAN, 16.0, NAN, 17.0]), np.array([NAN, NAN, 18.0, 19.0]))
    held0 = tuple(np.full(4, -1.0) for _ in range(7))
    blk = cref.fresh_block()
    assert all(same(a, b) for a, b in zip(cref.keep(blk, B, st, held0), held0))      # keep = 0: nothing
    cref.ints(blk)[cref.KEEP] = 1
    held = cref.keep(blk, B, st, held0)
    assert same(held[0], st[0]) and same(held[2], st[2]) and same(held[1], [-1.0, 5.0, 6.0, 7.0])
    assert same(held[3], [0.0, 12.0, 0.0, 13.0]) and same(held[4], [0.0, 0.0, 14.0, 15.0]) and same(held[5], [-1.0, 16.0, 0.0, 17.0]) and same(held[6], [-1.0, 0.0, 18.0, 19.0])
    poison = tuple(np.full(4, NAN) for _ in range(7))
    assert all(np.isnan(a).all() for a in cref.restore(blk, B, held, poison))      # kept = 0: nothing
    cref.ints(blk)[cref.KEPT] = 1
    back = cref.restore(blk, B, held, poison)
    assert all(same(a, b) for a, b in zip(back, st))      # NaN exactly where keep reads nothing
    # the maxima: −0.0, −NaN and −inf count by their absolute value; a NaN beats an infinity; empty: +0.0
    assert same(cref.xmax(np.array([-0.0, -3.0, 2.0])), 3.0) and same(cref.xmax(np.array([-INF, 1.0])), INF) and np.isnan(cref.xmax(np.array([INF, -NAN, 1.0])))
    assert same(cref.xmax(np.zeros(0)), 0.0)
    assert same(cref.check(cref.fresh_block(), words(1.0), 1.0, np.array([1.0, -5.0]), COUNTS, cref.options(), MO)[14], 5.0)
