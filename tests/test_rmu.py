"""The restoration phase's barrier parameter (iem_rmu_*, csrc/iem_rmu_device.h; iem_resto_bind_mu) — what needs no device: the symbols,
both source calls (the code object's own key, its five kernels, no float atomic, no inline assembly, no scratch; the bound variant
of the restoration code object: every edit matches, no host scalar is left, and the unbound source and key are what they were), the
refusals and the range table that come before any device work, and the restatement (tests/rmu_reference.py): every branch of
update, trigger and enter on hand-built words, the candidate words against resto_reference.error at each (mu_k, zeta_k), and the host
loop on the two Waechter-Biegler models and on the classical one."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mu_reference as mref
import resto_reference as rref
import rmu_reference as qref
import search_reference as sref

_HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = ("rmu_error", "rmu_enter", "rmu_update", "rmu_trigger", "rmu_gather")
CALLS = ("iem_rmu_create", "iem_rmu_destroy", "iem_rmu_mu", "iem_rmu_enter", "iem_rmu_error", "iem_rmu_update", "iem_rmu_trigger", "iem_rmu_device", "iem_rmu_state",
         "iem_resto_bind_mu", "iem_rmu_source", "iem_resto_mu_source")
RESTO_KEY = 0xb64b86a933ec1837      # iem_resto_source's key before the bound variant existed: the unbound code object is what it was
NAN = float("nan")
I = qref.ints
same = lambda a, b: np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.int64), np.ascontiguousarray(b, dtype=np.float64).view(np.int64))


def fnv(src):
    h = 1469598103934665603
    for byte in src.encode():
        h = ((h ^ byte) * 1099511628211) & (2 ** 64 - 1)
    return h


def test_symbols_and_bindings(built):
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.barrier import Restoration, RestorationParameter
    L = iemlib.lib()
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "iem.h")).read()
    for name in CALLS:
        assert name in iemlib.SYMBOLS and getattr(L, name).argtypes is not None and re.search(r"\bint " + name + r"\(", header), name
    assert C.sizeof(iemlib.RmuOpts) == 64 and C.sizeof(iemlib.RmuState) == 28 * 8
    o = iemlib.RmuOpts.defaults()
    assert {k: getattr(o, k) for k in qref.OPTS} == qref.OPTS == dict(kappa_eps=10.0, kappa_mu=0.2, tau_min=0.99, tol=1e-8, mu_floor=1e-11, s_max=100.0, gamma_alpha=0.05)
    assert iemlib.RMU_K == qref.K == 6 and "#define IEM_RMU_K 6" in header
    for method in ("enter", "error", "update", "trigger", "state", "device", "close", "__enter__", "__exit__"):
        assert callable(getattr(RestorationParameter, method)), method
    assert callable(Restoration.bind_mu)
    with pytest.raises(TypeError):
        iemlib.RmuOpts.defaults(kappa=0.5)
    assert iemlib.RMU_STATUS == ("iterating", "stationary", "unusable")
    assert "kept for a later restoration binding" not in header and "a binding for iem_resto" not in header


def test_the_source(built):
    """a code object of its own behind the helpers of the device header, compiled without contraction: the key is fnv1a64 of the text
    and no other object's, five kernels, no float atomic and no inline assembly in its own text"""
    from infiniteexamodels.jl_amd import lib as iemlib
    src, key = iemlib.rmu_source()
    assert iemlib.rmu_source() == (src, key) and key == fnv(src)
    others = [k for _, _, k in iemlib.fixed_sources()] + [f()[1] for f in (iemlib.search_source, iemlib.soc_source, iemlib.resto_source, iemlib.mu_source, iemlib.conv_source,
                                                                           iemlib.resto_mu_source)]
    assert key not in others
    head = src.split("\n", 1)[0]
    assert head.startswith("// iem-flags:") and "-ffp-contract=off" in head
    prefix, own = src.split("// iem_rmu_device.h", 1)
    assert "#define IEM_TILE 256" in prefix and "iem_shared_park" in prefix and "__global__" not in prefix
    kernels = re.findall(r"__global__ [^\n]*void (\w+)\(", own)
    assert tuple(kernels) == KERNELS and src.count("__global__") == len(KERNELS)
    code = "\n".join(line.split("//", 1)[0] for line in own.splitlines())
    assert set(re.findall(r"\batomic\w*\(", code)) == {"atomicMin(", "atomicMax("} and "asm" not in code and "iem_grad_atomic" not in code and "cooperative" not in code
    assert "#define RMU_K 6" in own


def test_the_bound_variant_of_the_restoration_source(built):
    """derived from the ONE text: every edit matched (the call succeeds), RestoArgs ends in the two pointers, no kernel reads a host
    scalar any more, everything else is the unbound text — and the unbound source and its key are what they were"""
    from infiniteexamodels.jl_amd import lib as iemlib
    src, key = iemlib.resto_source()
    assert key == RESTO_KEY == fnv(src)
    bound, bkey = iemlib.resto_mu_source()
    assert bkey == fnv(bound) and bkey != key and iemlib.resto_mu_source() == (bound, bkey)
    own = bound.split("// iem_resto_device.h", 1)[1]
    code = "\n".join(line.split("//", 1)[0] for line in own.splitlines())
    assert "const double *mu_blk, *mu_orig_blk;" in code
    assert not re.search(r"A\.(tau|zeta)\b", code) and re.findall(r"A\.mu\b[^_]", code) == ["A.mu)"]      # the one left: resto_check without an original block
    assert code.count("A.mu_blk[0]") == 6 and code.count("A.mu_blk[1]") == 1 and code.count("A.mu_blk[2]") == 5 and code.count("A.mu_orig_blk[0]") == 1
    assert re.findall(r"__global__ [^\n]*void (\w+)\(", bound) == re.findall(r"__global__ [^\n]*void (\w+)\(", src)
    # line for line: only the edited lines differ
    a, b = src.splitlines(), bound.splitlines()
    assert len(b) == len(a) + 1
    differ = [x for x in a if x not in b]
    assert len(differ) == 8, differ


@pytest.mark.skipif(not os.path.exists(_HIPCC), reason="no hipcc")
@pytest.mark.parametrize("which", ["rmu", "resto_mu"])
def test_the_objects_compile_without_scratch(which, built, tmp_path):
    from infiniteexamodels.jl_amd import lib as iemlib
    src, _ = iemlib.rmu_source() if which == "rmu" else iemlib.resto_mu_source()
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
    want = KERNELS if which == "rmu" else re.findall(r"__global__ [^\n]*void (\w+)\(", src)
    assert usage == {k: 0 for k in want}, usage


def test_refusals_and_the_range_table_need_no_device(built):
    from infiniteexamodels.jl_amd import lib as iemlib
    L = iemlib.lib()
    err = lambda: L.iem_last_error().decode()
    N = None
    out = C.c_void_p()
    assert L.iem_rmu_create(N, N, N, C.byref(out)) == -4 and "null" in err()
    assert L.iem_rmu_destroy(N) == 0
    assert L.iem_rmu_mu(N, N) == -4 and "null" in err()
    assert L.iem_rmu_enter(N, N, 0.1) == -4 and "null" in err()
    assert L.iem_rmu_error(N, *[N] * 10) == -4 and "null" in err()
    assert L.iem_rmu_update(N, N) == -4 and "null" in err()
    assert L.iem_rmu_trigger(N, 0, N) == -4 and "null" in err()
    assert L.iem_rmu_trigger(N, 2, N) == -4 and "which" in err()
    assert L.iem_rmu_device(N, N) == -4 and "null" in err()
    assert L.iem_rmu_state(N, N) == -4 and "null" in err()
    assert L.iem_resto_bind_mu(N, N) == -4 and "null" in err()
    # the range table: refused before the iem_resto object is looked at (the handle below is never dereferenced)
    fake = C.create_string_buffer(512)
    for name in qref.OPTS:
        bads = [0.0, -1.0, NAN, float("inf"), float("-inf")] + ([1.0, 1.5] if name in ("kappa_mu", "tau_min", "gamma_alpha") else [])
        for v in bads:
            o = iemlib.RmuOpts.defaults(**{name: v})
            assert L.iem_rmu_create(fake, N, C.byref(o), C.byref(out)) == -4 and name in err() and not out.value, (name, v)
    o = iemlib.RmuOpts.defaults()
    o.struct_size = 4
    assert L.iem_rmu_create(fake, N, C.byref(o), C.byref(out)) == -4 and "struct_size" in err()
    assert L.iem_rmu_create(fake, N, C.byref(iemlib.RmuOpts.defaults()), N) == -4 and "null" in err()


# ---- the restatement: update ---------------------------------------------------------------------------------------------------------
COUNTS = (3, 10)      # ncon, nz + 2·ncon


def words(mu0=0.1, d=(1.0,) * 6, dr=None, inf=0.0, pmax=None, pmin=None, bad=0.0, opts=qref.OPTS):
    """32 words by hand: candidates from mu0, the dual maxima `d` (variables) and `dr` (rows) per candidate, max |rc| = inf, and the
    products' extremes around mu0 unless given; sums small enough that sd = sc = 1"""
    blk = mref.fresh_block(dict(opts, mu_init=mu0))
    mu, _ = qref.ladder(blk, opts)
    w = np.zeros(32)
    w[2], w[4], w[5] = inf, 1.0, 2.0
    w[3] = mu0 if pmax is None else pmax
    w[8] = mu0 if pmin is None else pmin
    w[10] = bad
    dr = d if dr is None else dr
    for k in range(6):
        w[12 + 3 * k], w[13 + 3 * k], w[14 + 3 * k] = mu[k], d[k], dr[k]
    w[0], w[1] = d[0], dr[0]
    return w, blk


def run_update(w, blk, opts=qref.OPTS, own=None):
    own = qref.fresh_own() if own is None else own
    ictl = sref.block(status=sref.F_TYPE, count=7, flags=3, alpha=0.25)
    own, mblk, ictl2 = qref.update(own, blk, ictl, w, COUNTS, opts)
    emptied = sref.word(ictl2, sref.COUNT) == 0 and sref.word(ictl2, sref.FLAGS) == 0
    assert emptied == bool(I(own)[qref.FLAGS] & 1) and (emptied or same(ictl2, ictl)) and same(ictl2[:11], ictl[:11])      # the filter goes exactly when mu moved
    return own, mblk


def test_update_every_branch():
    # UNUSABLE by count and by NaN: nothing moves
    for w, blk in (words(bad=1.0), words(d=(NAN,) * 6), words(inf=NAN)):
        own, mblk = run_update(w, blk)
        assert I(own)[qref.STATUS] == qref.UNUSABLE and same(mblk, blk) and I(own)[qref.FLAGS] == 0 and I(own)[qref.LAST] == 0
    # STATIONARY: E_0(0) <= tol — products at 1e-9, the duals at 1e-9
    w, blk = words(mu0=1e-9, d=(1e-9,) * 6)
    own, mblk = run_update(w, blk)
    assert I(own)[qref.STATUS] == qref.STATIONARY and same(mblk, blk) and own[qref.E0] == 1e-9 and own[qref.E0] <= 1e-8
    # 0 decreases: the dual error is above kappa_eps·mu
    w, blk = words(mu0=0.1, d=(2.0,) * 6)
    own, mblk = run_update(w, blk)
    assert (I(own)[qref.STATUS], I(own)[qref.FLAGS], I(own)[qref.LAST], I(own)[qref.TOTAL]) == (0, 0, 0, 0) and same(mblk, blk)
    assert own[qref.E0] == 2.0 and own[qref.EMU] == 2.0
    # 1, 3 and 5 decreases: the dual maxima of the candidates decide where the ladder stops (the products sit at mu0: e_c(mu_k) = mu0 − mu_k <= mu0)
    mu, _ = qref.ladder(mref.fresh_block(dict(qref.OPTS, mu_init=0.1)))
    want = [0.1]
    for _ in range(5):
        want.append(max(1e-11, min(0.2 * want[-1], want[-1] * math.sqrt(want[-1]))))      # (0.2 mu first, mu^1.5 from the third candidate on)
    assert mu.tolist() == want and want[1] == 0.2 * 0.1 and want[3] == want[2] * math.sqrt(want[2]) and want[5] > 1e-11
    for stop in (1, 3, 5):
        # candidate k counts as solved iff its E <= 10 mu_k: the duals are 5 mu_k up to `stop` and 20 mu_k from there
        d = tuple((5.0 if k < stop else 20.0) * mu[k] for k in range(6))
        w, blk = words(mu0=0.1, d=d, pmax=0.0, pmin=0.0)      # (products at 0: e_c(mu) = mu, below 10 mu)
        own, mblk = run_update(w, blk)
        assert (I(own)[qref.STATUS], I(own)[qref.FLAGS], I(own)[qref.LAST], I(own)[qref.TOTAL]) == (0, 1, stop, stop), (stop, own[:4].view(np.int64))
        assert same(mblk[:3], [mu[stop], np.maximum(0.99, 1.0 - mu[stop]), np.sqrt(mu[stop])]) and same(mblk[3:], blk[3:])
        assert same(own[qref.EMU], max(d[stop], mu[stop])) and own[qref.E0] == d[0]
    # truncation: candidate 5 still counts as solved; the next update goes on from there
    d = tuple(5.0 * mu[k] for k in range(6))
    w, blk = words(mu0=0.1, d=d, pmax=0.0, pmin=0.0)
    own, mblk = run_update(w, blk)
    assert (I(own)[qref.FLAGS], I(own)[qref.LAST]) == (3, 5) and mblk[0] == mu[5]
    w2, _ = words(mu0=0.1, d=(1.0,) * 6)
    own2, mblk2 = run_update(*words(mu0=float(mblk[0]), d=(1.0,) * 6), own=own)
    assert (I(own2)[qref.FLAGS], I(own2)[qref.LAST], I(own2)[qref.TOTAL]) == (0, 0, 5)      # both flags describe the LAST update; the total stays
    # the floor: mu stops at mu_floor and a candidate at the floor is never left
    opts = dict(qref.OPTS, mu_floor=1e-3)
    w, blk = words(mu0=0.1, d=(1e-4,) * 6, pmax=0.0, pmin=0.0, opts=opts)
    assert w[12:30:3].tolist() == want[:3] + [1e-3, 1e-3, 1e-3]
    own, mblk = run_update(w, blk, opts)
    assert (I(own)[qref.FLAGS], I(own)[qref.LAST]) == (1, 3) and mblk[0] == 1e-3
    own, mblk2 = run_update(*words(mu0=1e-3, d=(1e-4,) * 6, pmax=0.0, pmin=0.0, opts=opts), opts)
    assert (I(own)[qref.FLAGS], I(own)[qref.LAST]) == (0, 0) and mblk2[0] == 1e-3
    # a NaN in a later candidate's maxima stops the ladder there (a NaN compares false)
    d = (1e-4, 1e-4, NAN, 1e-4, 1e-4, 1e-4)
    w, blk = words(mu0=0.1, d=d, pmax=0.0, pmin=0.0)
    own, mblk = run_update(w, blk)
    assert (I(own)[qref.STATUS], I(own)[qref.LAST]) == (0, 2) and np.isnan(own[qref.EMU])


# ---- the restatement: trigger --------------------------------------------------------------------------------------------------------
def trigger_cases():
    """``[(label, control block, fires)]``: every branch of alpha_min; each alpha lies at least a factor 2 away from alpha_min, so no
    decision hinges on the last bit of pow"""
    g = sref.OPTS
    out = []

    def add(label, fires, **kw):
        ctl = sref.block(**{**dict(alpha_max=1.0, phi0=3.0, theta_min=1e-4, theta_max=1e4, status=sref.SEARCHING, trials=3, flags=1, count=2), **kw})
        amin = float(qref.alpha_min(ctl))
        a = float(ctl[sref.ALPHA])
        if amin == amin:
            assert (a <= amin / 2.0) if fires else (a >= 2.0 * amin), (label, a, amin)
        out.append((label, ctl, fires))
    base = 0.05 * g["gamma_theta"]      # slope >= 0: alpha_min = gamma_alpha·gamma_theta = 5e-7
    add("slope >= 0, above", False, alpha=4.0 * base, theta0=2.0, slope=0.5)
    add("slope >= 0, below", True, alpha=0.25 * base, theta0=2.0, slope=0.5)
    add("slope = 0", True, alpha=0.25 * base, theta0=2.0, slope=0.0)
    # theta0 above theta_min: min(gamma_theta, gamma_phi·theta0/(−slope)) = 1e-8·2/4 = 5e-9; alpha_min = 2.5e-10
    add("theta0 above theta_min, above", False, alpha=1e-9, theta0=2.0, slope=-4.0)
    add("theta0 above theta_min, below", True, alpha=1e-10, theta0=2.0, slope=-4.0)
    add("theta0 above theta_min, gamma_theta decides", True, alpha=0.25 * base, theta0=2.0, slope=-1e-9)
    # theta0 below theta_min: the switching term delta·theta0^1.1/(−slope)^2.3 = (1e-6)^1.1/100^2.3 ~ 6.3e-12 decides against 1e-8·1e-6/100 = 1e-16?  no:
    # gamma_phi·theta0/(−slope) = 1e-16 is smaller — so a slope of −0.01 is used as well, where the switching term (1e-6)^1.1·(0.01)^-2.3 ~ 1e-2 loses too;
    # the table keeps both and the next two rows, where it wins: theta0 = 1e-6, slope = −1e6: 1e-8·1e-6/1e6 = 1e-20 against (1e-6)^1.1/(1e6)^2.3 ~ 4e-21
    add("theta0 below theta_min, the phi term decides, above", False, alpha=1e-16, theta0=1e-6, slope=-100.0)
    add("theta0 below theta_min, the phi term decides, below", True, alpha=1e-18, theta0=1e-6, slope=-100.0)
    add("theta0 below theta_min, the switching term decides, above", False, alpha=1e-21, theta0=1e-6, slope=-1e6)
    add("theta0 below theta_min, the switching term decides, below", True, alpha=2e-23, theta0=1e-6, slope=-1e6)
    add("NaN slope: gamma_theta alone", True, alpha=0.25 * base, theta0=2.0, slope=NAN)
    add("NaN slope, above", False, alpha=4.0 * base, theta0=2.0, slope=NAN)
    add("NaN theta0: alpha_min is a NaN and compares false", False, alpha=1e-30, theta0=NAN, slope=-1.0)
    for status in (sref.F_TYPE, sref.H_TYPE, sref.FAILED, sref.UNUSABLE):
        out.append((f"not SEARCHING ({status})", sref.block(alpha=1e-30, theta0=2.0, slope=-1.0, theta_min=1e-4, status=status), None))
    return out


def test_trigger_every_branch():
    g = sref.OPTS
    c = {label: (ctl, fires) for label, ctl, fires in trigger_cases()}
    # the switching term really decides where the label says so
    ctl = c["theta0 below theta_min, the switching term decides, above"][0]
    sw = (g["delta"] * np.power(1e-6, g["s_theta"])) / np.power(1e6, g["s_phi"])
    assert sw < (g["gamma_phi"] * 1e-6) / 1e6 < g["gamma_theta"] and same(qref.alpha_min(ctl), 0.05 * sw)
    ctl = c["theta0 below theta_min, the phi term decides, above"][0]
    assert same(qref.alpha_min(ctl), 0.05 * ((g["gamma_phi"] * 1e-6) / 100.0))
    for which in (0, 1):
        own0 = qref.fresh_own()
        own0[qref.ALPHA_MIN] = 77.0
        I(own0)[qref.TRIG_ORIG], I(own0)[qref.TRIG_INNER] = 4, 9
        for label, (ctl, fires) in c.items():
            own, ctl2, a0 = qref.trigger(own0, ctl, which)
            if fires is None:
                assert same(own, own0) and same(ctl2, ctl) and a0 is None, label
                continue
            assert same(own[qref.ALPHA_MIN], qref.alpha_min(ctl)), label
            counters = (int(I(own)[qref.TRIG_ORIG]), int(I(own)[qref.TRIG_INNER]))
            if fires:
                assert sref.word(ctl2, sref.STATUS) == sref.FAILED and same(ctl2[sref.ALPHA], 0.0) and same(a0, 0.0) and same(ctl2[1:9], ctl[1:9]) and same(ctl2[10:], ctl[10:]), label
                assert counters == ((5, 9) if which == 0 else (4, 10)), label
                again = qref.trigger(own, ctl2, which)      # idempotent
                assert same(again[0], own) and same(again[1], ctl2) and again[2] is None, label
            else:
                assert same(ctl2, ctl) and a0 is None and counters == (4, 9), label
                again = qref.trigger(own, ctl2, which)
                assert same(again[0], own) and same(again[1], ctl2), label


# ---- the restatement: enter ----------------------------------------------------------------------------------------------------------
def test_enter_every_branch():
    opts = qref.OPTS
    own0 = np.arange(16, dtype=np.float64) + 1.0
    mblk0 = mref.fresh_block(dict(opts, mu_init=0.3))
    mblk0[3:8] = [1.0, 2.0, 3.0, 4.0, 5.0]
    mref.ints(mblk0)[8:12] = [2, 1, 7, 9]
    ictl0 = sref.block(status=sref.F_TYPE, count=7, flags=3, alpha=0.25, theta_min=1e-4)
    err = lambda inf: np.array([9.0, 9.0, inf, 9.0, 9.0, 9.0, 9.0, 9.0])
    oblk = mref.fresh_block(dict(opts, mu_init=0.02))
    for label, e, mu_host, ob, want in (("the infeasibility decides", err(2.5), 0.1, None, 2.5), ("mu decides", err(0.01), 0.1, None, 0.1),
                                        ("the original block's mu, not the host's", err(0.01), 0.1, oblk, 0.02), ("the original block, the infeasibility decides", err(0.5), 7.0, oblk, 0.5)):
        own, mblk, ictl = qref.enter(own0, mblk0, ictl0, e, mu_host, ob)
        assert same(mblk, mref.reset(mblk0, dict(opts, mu_init=0.1), want)) and same(mblk[:3], [want, max(0.99, 1.0 - want), np.sqrt(want)]), label
        assert same(mblk[3:8], mblk0[3:8]) and not mref.ints(mblk)[8:12].any(), label
        expect = np.zeros(16)
        expect[qref.MU_ENTER], expect[qref.INF_ENTER] = want, e[2]
        assert same(own, expect), label
        assert sref.word(ictl, sref.COUNT) == 0 and sref.word(ictl, sref.FLAGS) == 0 and same(ictl[:11], ictl0[:11]), label
    for label, e, mu_host, ob in (("a NaN infeasibility", err(NAN), 0.1, None), ("a NaN mu", err(0.5), NAN, None), ("not positive", err(0.0), 0.0, None),
                                  ("negative", err(-1.0), -2.0, None), ("a NaN in the original block", err(0.5), 0.1, np.full(16, NAN))):
        own, mblk, ictl = qref.enter(own0, mblk0, ictl0, e, mu_host, ob)
        expect = own0.copy()
        I(expect)[qref.STATUS] = qref.UNUSABLE
        assert same(own, expect) and same(mblk, mblk0) and same(ictl, ictl0), label


# ---- the candidate words against resto_reference.error ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["opf_7", "pandemic_20x3", "wb_eq", "wb_ineq"])
def test_the_candidate_words(name, built):
    """[12 + 3k] is the ladder, [13 + 3k], [14 + 3k] are out[0], out[1] of resto_reference.error at (mu_k, zeta_k) — which do not depend
    on mu —, [0..7] the eight numbers at (0, zeta_0), [8..10] the products' minimum, sum and unusable count with p·zp, n·zn among them"""
    P = rref.point(name)
    B = P["B"]
    R, st, mu = rref.entered(P)
    r = P["om"].jtprod(st[0], st[2])
    mblk = mref.fresh_block(dict(qref.OPTS, mu_init=mu))
    w = qref.error_words(B, R, st, r, P["c"], mblk)
    mus, zetas = qref.ladder(mblk)
    assert same(w[12:30:3], mus) and (np.diff(mus) < 0).all() and same(zetas[1:], np.sqrt(mus[1:])) and same(zetas[0], mblk[2])
    for k in range(6):
        head, ay, mult, theta, logs = rref.error(B, R, st, r, P["c"], float(mus[k]), float(zetas[k]))
        assert same(w[13 + 3 * k:15 + 3 * k], head[:2]), k
    head0, ay, mult, theta, logs = rref.error(B, R, st, r, P["c"], 0.0, float(zetas[0]))
    assert same(w[:4], head0) and same(w[4:8], [ay.sum(), mult.sum(), theta.sum(), logs.sum()])
    p = qref.products(B, R, st)
    assert len(p) == B["counts"]["nz"] + 2 * len(P["c"]) and same(w[8], p.min()) and same(w[9], p.sum()) and w[10] == 0.0 and (p > 0).all()
    assert same(w[3], np.abs(p).max()) and not w[11] and not w[30:].any()
    # the zeta term matters: the candidates' dual maxima are not all the same
    assert len({float(v) for v in w[13:30:3]}) > 1 or len({float(v) for v in w[14:30:3]}) > 1
    # the device's order on one workgroup-sized grid carries the same maxima and counts
    wd = qref.error_device(B, R, st, r, P["c"], mblk, bref_grid(len(st[0]) + len(st[2])))
    assert same(wd[:4], w[:4]) and same(wd[8], w[8]) and same(wd[10], w[10]) and same(wd[12:30], w[12:30]) and np.allclose(wd[4:10], w[4:10], rtol=1e-12, atol=0)
    # a negative product and a NaN product: counted, kept out of the minimum
    bad = [a.copy() for a in st]
    Rb = {k: v.copy() for k, v in R.items()}
    Rb["zp"][0] = -Rb["zp"][0]
    Rb["zn"][-1] = NAN
    wb = qref.error_words(B, Rb, tuple(bad), r, P["c"], mblk)
    assert wb[10] == 2.0 and same(wb[8], np.delete(p, [len(p) - 2 * len(P["c"]), len(p) - 1]).min()) and np.isnan(wb[9]) and np.isnan(wb[3])


def bref_grid(n):
    import barrier_reference as bref
    return bref.grid(n)


# ---- the host loop ---------------------------------------------------------------------------------------------------------------------
def _classical():
    from infiniteexamodels.jl_amd import transcribe
    from pyoracle import OracleModel
    return OracleModel(transcribe.exa_core(rref.wachter_biegler(-1.0, 0.5, 3, False, start=(-2.0, 3.0, 1.0))).to_blob())


@pytest.mark.parametrize("name", list(rref.WB_MODELS))
def test_the_host_loop_solves_with_fewer_accepts(name, built):
    """solved, the same restorations (and iterates, bit for bit) as the loop without the rule, fewer accept calls with the trigger"""
    from pyoracle import OracleModel
    om = OracleModel(rref.wb_core(name).to_blob())
    base = rref.host_loop(om)
    without = qref.host_loop(om, use_trigger=False)
    got = qref.host_loop(om)
    show = lambda o: {k: o[k] for k in ("status", "iterations", "error", "objective", "restorations", "resto_iterations", "why", "accepts", "decreases", "truncated", "triggers")}
    print(name, "without the trigger:", show(without))
    print(name, "with the trigger:   ", show(got))
    optimum = rref.WB_MODELS[name]["optimum"]
    for o in (without, got):
        assert o["status"] == "solved" and o["error"] <= 1e-8 and abs(o["objective"] / optimum - 1.0) <= 1e-6
        assert (o["iterations"], o["restorations"], o["resto_iterations"]) == (base["iterations"], base["restorations"], base["resto_iterations"]) and base["restorations"] >= 1
        assert not o["truncated"] and max(o["decreases"]) <= 5 and same(o["x"], base["x"])
    assert len(got["iterates"]) == len(without["iterates"]) and all(same(a, b) for a, b in zip(got["iterates"], without["iterates"]))
    assert got["accepts"] < without["accepts"] and got["triggers"][0] >= 1 and without["triggers"] == (0, 0)


def test_the_classical_model_ends_stationary(built):
    """a = −1, b = 0.5 from (−2, 3, 1): the restoration converges to a local minimiser of the infeasibility — reported as such
    (STATIONARY), no longer as a failed inner search; the cap of five decreases per update is never reached"""
    om = _classical()
    base = rref.host_loop(om)
    assert base["status"] == "restoration failed" and base["why"] == "inner search failed"
    without = qref.host_loop(om, use_trigger=False)
    got = qref.host_loop(om)
    for o in (without, got):
        print({k: o[k] for k in ("status", "iterations", "error", "restorations", "resto_iterations", "why", "accepts", "decreases", "truncated", "triggers")}, o["e0"][-3:])
        assert o["status"] == "locally infeasible" and o["why"] == "stationary" and o["error"] > 1e-8 and o["iterations"] == base["iterations"]
        assert not o["truncated"] and 1 <= max(o["decreases"]) <= 5 and o["e0"][-1] <= 1e-8 < o["e0"][-2]
    assert got["accepts"] < without["accepts"] and all(same(a, b) for a, b in zip(got["iterates"], without["iterates"]))
