"""The starting point's arithmetic and refusals without a GPU: tests/init_reference.py (the numpy restatement of
csrc/iem_init_device.h) against numpy.linalg.lstsq, tests/barrier_reference.py and tests/mu_reference.py.

(a) symbols, struct sizes, the defaults stated twice, the refusals that need no device;
(b) the source: a code object of its own behind the helpers, the integer maximum its only atomic call, no scratch;
(c) the normal equations: the K of iem_init_ls_terms gives numpy's least-squares multipliers and does not raise the objective;
(d) every branch of ls_apply;
(e) warm: each clamp on each side, NaN multipliers, every kind of bound pair, the warm_frac branch, equality rows untouched;
(f) mu: all four values of word 5, mu_cap = 0, the block of mu_reference.reset."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import barrier_reference as bref
import init_reference as iref
import mu_reference as mref

_HIPCC = "/opt/rocm/bin/hipcc"
CALLS = ("iem_init_create", "iem_init_destroy", "iem_init_reset", "iem_init_ls_terms", "iem_init_ls_apply", "iem_init_warm", "iem_init_mu", "iem_init_device",
         "iem_init_state", "iem_init_source")
KERNELS = ("init_ls_apply", "init_ls_norm", "init_ls_terms", "init_mu", "init_reset", "init_warm")
NAN, INF = float("nan"), float("inf")


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def test_symbols_and_bindings(built):
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.barrier import StartingPoint
    L = iemlib.lib()
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "iem.h")).read()
    for name in CALLS:
        assert name in iemlib.SYMBOLS and getattr(L, name).argtypes is not None and re.search(r"\bint " + name + r"\(", header), name
    assert C.sizeof(iemlib.InitOpts) == 10 * 8 and C.sizeof(iemlib.InitState) == 7 * 8
    assert iemlib.InitOpts._fields_[0][0] == "struct_size" and iemlib.InitState._fields_[0][0] == "struct_size"
    o = iemlib.InitOpts.defaults()
    assert {k: getattr(o, k) for k in iref.OPTS} == iref.OPTS == iemlib.InitOpts.DEFAULTS      # the defaults, stated twice
    for method in ("reset", "ls_terms", "ls_apply", "warm", "mu", "state", "device", "close", "__enter__", "__exit__"):
        assert callable(getattr(StartingPoint, method)), method
    with pytest.raises(TypeError):
        iemlib.InitOpts.defaults(bound_push=0.5)
    assert len(iemlib.INIT_HOW) == 4


def test_the_source(built):
    """a code object of its own behind the helpers, compiled without contraction: the same text and key twice, the key fnv1a64 of the
    text and no other object's, its own six kernels (the four calls' among them), the integer maximum as the only atomic call of its
    own text, no inline assembly; no other object's source knows of it and the fixed sources are the three they were"""
    from infiniteexamodels.jl_amd import lib as iemlib
    src, key = iemlib.init_source()
    assert iemlib.init_source() == (src, key)
    h = 1469598103934665603
    for byte in src.encode():
        h = ((h ^ byte) * 1099511628211) & (2 ** 64 - 1)
    assert key == h
    fixed = list(iemlib.fixed_sources())
    assert len(fixed) == 3
    siblings = (iemlib.search_source, iemlib.soc_source, iemlib.resto_source, iemlib.mu_source, iemlib.barrier_mu_source, iemlib.amu_source, iemlib.qf_source,
                iemlib.mpc_source)
    others = [k for _, _, k in fixed] + [f()[1] for f in siblings]
    assert key not in others and len(set(others)) == len(others)
    assert all(text != src for _, text, _ in fixed)
    head = src.split("\n", 1)[0]
    assert head.startswith("// iem-flags:") and "-ffp-contract=off" in head
    prefix, own = src.split("// iem_init_device.h", 1)
    assert "#define IEM_TILE 256" in prefix
    kernels = re.findall(r"__global__ [^\n]*void (\w+)\(", own)
    assert tuple(sorted(kernels)) == KERNELS and src.count("__global__") == len(KERNELS)
    assert {"init_ls_terms", "init_ls_apply", "init_warm", "init_mu"} <= set(kernels)
    code = "\n".join(line.split("//", 1)[0] for line in own.splitlines())
    assert re.findall(r"\batomic\w*\(", code) == ["atomicMax("]      # ONE call site, on 64-bit integers: no atomicAdd on a float
    assert re.findall(r"__hip_atomic\w*", code) == ["__hip_atomic_load"]      # the relaxed look at the slot in front of it
    assert "atomicAdd" not in code and "asm" not in code and "cooperative" not in code and "grid.sync" not in code
    assert "iem_grad_atomic(" not in code and "iem_grad_wave_uniform(" not in code      # the helpers' float atomics stay unused
    for f in siblings + (iemlib.barrier_source,):
        assert "init_ls_" not in f()[0] and "init_warm" not in f()[0]
    assert all("init_ls_" not in text for _, text, _ in fixed)


@pytest.mark.skipif(not os.path.exists(_HIPCC), reason="no hipcc")
def test_the_object_compiles_without_scratch(built, tmp_path):
    from infiniteexamodels.jl_amd import lib as iemlib
    src, _ = iemlib.init_source()
    head = src.split("\n", 1)[0]
    hip = tmp_path / "i.hip"
    hip.write_text(src)
    p = subprocess.run([_HIPCC, "--genco", "--offload-arch=gfx950", *head[len("// iem-flags:"):].split(), "-Rpass-analysis=kernel-resource-usage",
                        "-o", str(tmp_path / "i.hsaco"), str(hip)], capture_output=True, text=True)
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
    assert L.iem_init_create(N, N, C.byref(out)) == -4 and "null" in err()
    assert L.iem_init_create(N, C.byref(iemlib.InitOpts.defaults()), N) == -4 and "null" in err()
    assert L.iem_init_destroy(N) == 0
    assert L.iem_init_reset(N) == -4 and "null" in err()
    assert L.iem_init_ls_terms(N, *[N] * 9) == -4 and "null" in err()
    assert L.iem_init_ls_apply(N, N, N) == -4 and "null" in err()
    assert L.iem_init_warm(N, *[N] * 7) == -4 and "null" in err()
    assert L.iem_init_mu(N, N, N) == -4 and "null" in err()
    assert L.iem_init_device(N, N) == -4 and "null" in err()
    assert L.iem_init_state(N, N) == -4 and "null" in err()


# ---- (c) the normal equations -----------------------------------------------------------------------------------------------------------
def _core(name):
    import cases
    from infiniteexamodels.jl_amd import transcribe
    if name == "rosenbrock":
        return transcribe.exa_core(cases.rosenbrock()[0])
    if name == "pfun":
        return transcribe.exa_core(cases.pfun()[0])
    return cases.build_core(name)


@pytest.mark.parametrize("name,written", [("rosenbrock", 2.2e-16), ("ode_5x5", 1.8e-14), ("pfun", 1.3e-15)])
def test_the_normal_equations(name, written, built):
    """The K of the contract — a zero Hessian, sigma = 1, dcon = 1 on inequality rows, delta_w = delta_c = 0 — built densely from the
    restated ls_terms at the cold start of the model (barrier_reference.start at x0, y = 0) and solved by numpy: y + delta is the
    minimiser numpy.linalg.lstsq finds for the stacked problem.  Both sides are numpy's, so the tolerance is numpy's own spread:
    d_ref = max |lstsq − solve(A'A, −A'b)|, its two routes to that minimiser, measured here on the same model; the K route may
    differ from lstsq by 16·d_ref (the factor tests/test_kkt_border.py grants a backward error).  The d_ref this was written with
     is printed beside what was found.  And the estimate does not raise the least-squares objective."""
    from pyoracle import OracleModel
    om = OracleModel(_core(name).to_blob())
    B, st, r, J = iref.cold_point(om)
    n = om.nvar
    assert not st[2].any() and B["counts"]["n_ineq"] > 0
    sigma, dcon, rhs = iref.ls_terms(B, st, r)
    assert same(sigma, np.ones(n)) and same(dcon, np.where(B["eq"], 0.0, 1.0)) and same(rhs[n:][B["eq"]], np.zeros(B["counts"]["n_eq"]))
    sol = iref.ls_solve(B, st, r, J)
    y_new = st[2] + sol[n:]
    by_svd, by_normal = iref.ls_lstsq(B, st, r, J)
    d_ref = float(np.abs(by_svd - by_normal).max())
    diff = float(np.abs(y_new - (st[2] + by_svd)).max())
    f_new, f_old = iref.ls_objective(B, st, r, J, sol[n:]), iref.ls_objective(B, st, r, J, np.zeros(om.ncon))
    print(f"{name}: nvar {n} ncon {om.ncon} d_ref {d_ref:.3e} (written with {written:.1e}) |K route - lstsq| {diff:.3e} max|y_new| {np.abs(y_new).max():.6g} "
          f"objective at y {f_old:.6g} at y_new {f_new:.6g}")
    assert d_ref > 0.0 and diff <= 16.0 * d_ref, (diff, d_ref)
    assert f_new <= f_old
    # w, the x part of the solution, is the residual of the first block: w = −(r − zL + zU) − J'delta
    z = lambda a, on: np.where(on, a, 0.0)
    w = -(r - z(st[3], B["hasL"]) + z(st[4], B["hasU"])) - J.T @ sol[n:]
    assert np.abs(sol[:n] - w).max() <= 1e-12 * max(1.0, np.abs(w).max())


# ---- (d) ls_apply -----------------------------------------------------------------------------------------------------------------------
def test_every_branch_of_ls_apply(built):
    nvar = 3
    y = np.array([1.0, -2.0, 0.5, 4.0])
    d = np.array([0.25, -1.0, 2.0, -0.5])
    sol = lambda dy, poison=NAN: np.concatenate([np.full(nvar, poison), dy])      # the x part is never read
    yn = y + d
    top = float(np.abs(yn).max())
    blk = iref.fresh_block()
    n_a = n_r = 0
    cases_ = [("accepted", iref.options(), d, True, yn), ("rejected by size, y = 0", iref.options(y_max=top / 2), d, False, np.zeros(4)),
              ("rejected by size, y kept", iref.options(y_max=top / 2, on_reject=1), d, False, y),
              ("rejected by NaN, y = 0", iref.options(), np.array([0.25, NAN, 2.0, -0.5]), False, np.zeros(4)),
              ("rejected by NaN, y kept", iref.options(on_reject=1), np.array([0.25, NAN, 2.0, -0.5]), False, y),
              ("rejected by inf", iref.options(y_max=1e300), np.array([0.25, INF, 2.0, -0.5]), False, np.zeros(4)),
              ("ynorm == y_max exactly", iref.options(y_max=top), d, True, yn),
              ("the next double below", iref.options(y_max=float(np.nextafter(top, 0.0))), d, False, np.zeros(4)),
              ("y_max = 0 with a zero estimate", iref.options(y_max=0.0), -y, True, np.zeros(4)),
              ("accepted with on_reject = 1", iref.options(on_reject=1), d, True, yn)]
    for label, o, dy, accepted, want in cases_:
        blk, got = iref.ls_apply(blk, y, sol(dy), nvar, o)
        n_a, n_r = n_a + accepted, n_r + (not accepted)
        iw = iref.ints(blk)
        assert (iw[iref.ACCEPTED], iw[iref.N_ACCEPTED], iw[iref.N_REJECTED]) == (int(accepted), n_a, n_r), label
        assert same(got, want), (label, got, want)
        with np.errstate(invalid="ignore"):
            assert same(blk[iref.YNORM], np.abs(y + dy).max()) or np.isnan(blk[iref.YNORM]) and np.isnan(dy).any(), label
        assert not blk[4:].any()
    assert n_a == 4 and n_r == 6
    # a NaN beats every number, an infinity included: the integer maximum on the bit patterns
    _, ynorm = iref.ls_norm(np.zeros(3), np.array([INF, NAN, -INF]), 0)
    assert np.isnan(ynorm)
    # −NaN and −0.0 count by their absolute value
    _, ynorm = iref.ls_norm(np.zeros(2), np.array([-0.0, -3.0]), 0)
    assert same(ynorm, 3.0)
    # ncon == 0: the norm is +0.0, the estimate is accepted, y stays empty
    blk0, y0 = iref.ls_apply(iref.fresh_block(), np.zeros(0), np.full(nvar, NAN), nvar, iref.options(y_max=0.0))
    assert same(blk0[iref.YNORM], 0.0) and iref.ints(blk0)[iref.ACCEPTED] == 1 and iref.ints(blk0)[iref.N_ACCEPTED] == 1 and len(y0) == 0


# ---- (e) warm ---------------------------------------------------------------------------------------------------------------------------
def _warm_case():
    """six variables — none, lower, upper, both wide, both narrower than 2·warm_push, both with the point outside — and five rows:
    an equality, lower, upper, both, both narrow"""
    inf = INF
    lvar = np.array([-inf, 1.0, -inf, 0.0, 2.0, -5.0])
    uvar = np.array([inf, inf, 3.0, 10.0, 2.0 + 1e-4, 5.0])
    lcon = np.array([1.5, 0.0, -inf, -1.0, 4.0])
    ucon = np.array([1.5, inf, 2.0, 1.0, 4.0 + 1e-4])
    return bref.relaxed_bounds(lvar, uvar, lcon, ucon, 0.0)


def test_warm(built):
    B = _warm_case()
    o = iref.options()
    k1, zp, zm, ym = o["warm_push"], o["warm_z_push"], o["warm_z_max"], o["warm_y_max"]
    assert B["eq"].tolist() == [True, False, False, False, False]
    x = np.array([NAN, 1.0, 3.5, 5.0, 2.00005, -7.0])      # free (never read: NaN stays), on the bound, outside, interior, narrow, outside below
    s = np.array([NAN, -1.0, 2.0, 0.25, 4.00002])
    y = np.array([2e6, -2e6, NAN, 0.5, -ym])
    zL = np.array([NAN, 1e-9, NAN, NAN, 2.0, 1e7])          # below the push, absent, a NaN at a present bound, inside, above the cap
    zU = np.array([NAN, NAN, 1e7, 1e-3, -1.0, 1e6])         # absent, absent, above, exactly the push, negative, exactly the cap
    vL = np.array([NAN, NAN, 7.0, 1e-9, 3.0])               # the equality row, a NaN at a present bound, absent, below, inside
    vU = np.array([NAN, 5.0, 1e9, INF, -INF])               # the equality row, absent, above, +inf, −inf
    xw, sw, yw, zLw, zUw, vLw, vUw = iref.warm(B, (x, s, y, zL, zU, vL, vU), o)
    # the primal push: barrier_reference.push with the warm constants; the free variable keeps its bits
    assert same(xw, bref.push(x, B["xl"], B["xu"], B["hasL"], B["hasU"], k1, o["warm_frac"])) and np.isnan(xw[0])
    assert same(xw[1], 1.0 + k1 * 1.0) and same(xw[2], 3.0 - k1 * 3.0) and same(xw[3], 5.0) and same(xw[5], -5.0 + k1 * 5.0)
    width = B["xu"][4] - B["xl"][4]
    assert width < 2 * k1 * 2.0 and same(xw[4], 2.00005)      # the interval narrower than 2·warm_push: pl = pu = warm_frac·width, the interior point stays
    lo, hi = B["xl"][4] + o["warm_frac"] * width, B["xu"][4] - o["warm_frac"] * width
    outside = iref.warm(B, (np.array([NAN, 1.0, 3.5, 5.0, 1.0, -7.0]), s, y, zL, zU, vL, vU), o)[0][4]
    assert same(outside, lo) and lo < hi
    # s: the same projection of THE GIVEN s; the equality row untouched
    assert np.isnan(sw[0]) and same(sw[1], 0.0 + k1) and same(sw[2], 2.0 - k1 * 2.0) and same(sw[3], 0.25) and same(sw[4], 4.00002)
    # the multipliers
    assert same(zLw, [0.0, zp, 0.0, zp, 2.0, zm]) and same(zUw, [0.0, 0.0, zm, zp, zp, 1e6])
    assert np.isnan(vLw[0]) and np.isnan(vUw[0])      # equality row: neither read nor written
    assert same(vLw[1:], [zp, 0.0, zp, 3.0]) and same(vUw[1:], [0.0, zm, zm, zp])
    # y on EVERY row, the equality row included: each side, a NaN, inside, exactly the limit
    assert same(yw, [ym, -ym, 0.0, 0.5, -ym])
    # with the constants of iem_barrier_start and s = c the primal side is barrier_reference.start, bit for bit
    P = bref.barrier_point("opf_7")
    Bp, stp = P["B"], P["state"]
    c = P["c"]
    far = stp[0] + 50.0 * np.sign(stp[0])      # a point far outside its bounds
    poison = tuple(np.full(len(c), NAN) for _ in range(3))
    xs, ss, *_ = bref.start(Bp, far, c, poison)
    got = iref.warm(Bp, (far, np.where(Bp["eq"], NAN, c), stp[2], *stp[3:]), iref.options(warm_push=bref.PUSH, warm_frac=bref.FRAC))
    assert same(got[0], xs) and same(got[1], ss) and not same(got[0], far)


# ---- (f) mu -----------------------------------------------------------------------------------------------------------------------------
def test_every_branch_of_mu(built):
    mo = mref.options()
    nz = 8
    w = np.zeros(12)
    mu_blk = mref.fresh_block(mo)
    mu_blk[3:8] = [1.0, 2.0, 3.0, 4.0, 5.0]
    mref.ints(mu_blk)[8:12] = [1, 1, 7, 9]      # a finished solve: CONVERGED, the flag, counters
    seen = {}
    cases_ = [("average", iref.options(), 8 * 1e-3, 0.0, 1e-3, iref.FROM_AVERAGE), ("NaN product counted", iref.options(), 8 * 1e-3, 1.0, mo["mu_init"], iref.FALLBACK),
              ("a NaN count", iref.options(), 8 * 1e-3, NAN, mo["mu_init"], iref.FALLBACK), ("a NaN sum", iref.options(), NAN, 0.0, mo["mu_init"], iref.FALLBACK),
              ("a zero sum", iref.options(), 0.0, 0.0, mo["mu_init"], iref.FALLBACK), ("a negative sum", iref.options(), -1.0, 0.0, mo["mu_init"], iref.FALLBACK),
              ("below the floor", iref.options(), 8 * 1e-12, 0.0, mo["mu_floor"], iref.CLAMPED_BELOW),
              ("above the cap: mu_cap = 0 takes mu_init", iref.options(), 8 * 5.0, 0.0, mo["mu_init"], iref.CLAMPED_ABOVE),
              ("above mu_cap", iref.options(mu_cap=0.5), 8 * 5.0, 0.0, 0.5, iref.CLAMPED_ABOVE), ("under mu_cap, above mu_init", iref.options(mu_cap=0.5), 8 * 0.25, 0.0, 0.25, iref.FROM_AVERAGE),
              ("exactly the cap", iref.options(mu_cap=0.5), 8 * 0.5, 0.0, 0.5, iref.FROM_AVERAGE), ("an infinite sum", iref.options(), INF, 0.0, mo["mu_init"], iref.CLAMPED_ABOVE),
              ("mu_factor", iref.options(mu_factor=0.5), 8 * 1e-3, 0.0, 0.5 * 1e-3, iref.FROM_AVERAGE)]
    blk = iref.fresh_block()
    for label, o, w9, w10, mu0, how in cases_:
        w[9], w[10] = w9, w10
        blk, got = iref.mu(blk, mu_blk, w, nz, o, mo)
        assert same(blk[iref.MU0], mu0) and iref.ints(blk)[iref.HOW] == how, (label, blk[:6])
        assert same(got, mref.reset(mu_blk, mo, mu0)), label      # the block of mu_reference's reset at the same mu0
        assert same(got[3:8], mu_blk[3:8]) and not mref.ints(got)[8:12].any() and same(got[:3], mref.fresh_block(mo, mu0)[:3])
        assert not blk[:4].any() and not blk[6:].any()
        seen[how] = seen.get(how, 0) + 1
    assert set(seen) == {0, 1, 2, 3}
    w[9], w[10] = 8 * 1e-3, 0.0
    assert iref.choose_mu(w, 0, iref.options(), mo) == (mo["mu_init"], iref.FALLBACK)      # nz = 0: no division
    other = mref.options(mu_init=0.01)
    assert iref.choose_mu(np.array([0.0] * 9 + [8 * 5.0, 0.0, 0.0]), nz, iref.options(), other) == (0.01, iref.CLAMPED_ABOVE)
