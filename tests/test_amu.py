"""The adaptive barrier parameter object's arithmetic and refusals without a GPU: tests/amu_reference.py (the numpy restatement of
csrc/iem_amu_device.h) against tests/mu_reference.py and tests/barrier_reference.py.

(a) every entry of `branch_cases` reaches the branch its label names;
(b) in FIXED mode without progress the rule IS the monotone rule: mu, tau, zeta and the decreases of mu_reference.update, bit for bit;
(c) on a state whose products are all equal LOQO gives sigma = +0.0, hence mu_min;
(d) with zero directions and alpha = (1, 1) the probe's terms are the complementarity products;
(e) the source: a code object of its own behind the helpers, no float atomic; the C-ABI's refusals with null handles."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import amu_reference as aref
import barrier_reference as bref
import mu_reference as mref

_HIPCC = "/opt/rocm/bin/hipcc"
CALLS = ("iem_amu_create", "iem_amu_destroy", "iem_amu_reset", "iem_amu_probe", "iem_amu_update", "iem_amu_device", "iem_amu_state", "iem_amu_source")
KERNELS = ("amu_probe", "amu_reset", "amu_update")
COUNTS = [(31, 17), (0, 5), (4, 0)]


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


def word_vector(P, st):
    """the twelve words with the sums in numpy's order (any one order serves the CPU tests)"""
    head, sums, w8, w10, p = mref.error_words(P["B"], st, P["r"], P["c"])
    return np.array([*head, *(float(np.sum(t)) for t in sums), w8, float(np.sum(p)), w10, 0.0])


def test_symbols_and_bindings(built):
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.barrier import AdaptiveBarrierParameter
    L = iemlib.lib()
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "iem.h")).read()
    for name in CALLS:
        assert name in iemlib.SYMBOLS and getattr(L, name).argtypes is not None and re.search(r"\bint " + name + r"\(", header), name
    assert C.sizeof(iemlib.AmuOpts) == 64 and C.sizeof(iemlib.AmuState) == 15 * 8
    assert iemlib.AmuOpts._fields_[0][0] == "struct_size" and iemlib.AmuState._fields_[0][0] == "struct_size"
    o = iemlib.AmuOpts.defaults()
    assert {k: getattr(o, k) for k in aref.OPTS} == aref.OPTS      # the defaults, stated twice
    assert iemlib.AmuOpts.defaults(oracle="loqo").oracle == aref.LOQO
    for method in ("probe", "update", "reset", "state", "device", "affine", "close", "__enter__", "__exit__"):
        assert callable(getattr(AdaptiveBarrierParameter, method)), method
    with pytest.raises(TypeError):
        iemlib.AmuOpts.defaults(kappa=0.5)
    with pytest.raises(ValueError):
        iemlib.AmuOpts.defaults(oracle="mehrotra")


def test_the_source(built):
    """a code object of its own behind the helpers, compiled without contraction: the same text and key twice, the key fnv1a64 of the
    text and no other object's, three kernels, no float atomic (no atomic at all in its own text), no inline assembly of its own"""
    from infiniteexamodels.jl_amd import lib as iemlib
    src, key = iemlib.amu_source()
    assert iemlib.amu_source() == (src, key)
    h = 1469598103934665603
    for byte in src.encode():
        h = ((h ^ byte) * 1099511628211) & (2 ** 64 - 1)
    assert key == h
    others = [k for _, _, k in iemlib.fixed_sources()] + [f()[1] for f in (iemlib.search_source, iemlib.soc_source, iemlib.resto_source, iemlib.mu_source, iemlib.barrier_mu_source)]
    assert key not in others and len(set(others)) == len(others)
    head = src.split("\n", 1)[0]
    assert head.startswith("// iem-flags:") and "-ffp-contract=off" in head
    prefix, own = src.split("// iem_amu_device.h", 1)
    assert "#define IEM_TILE 256" in prefix and "iem_shared_park" in prefix
    kernels = re.findall(r"__global__ [^\n]*void (\w+)\(", own)
    assert tuple(sorted(kernels)) == KERNELS and src.count("__global__") == len(KERNELS)
    code = "\n".join(line.split("//", 1)[0] for line in own.splitlines())
    assert re.findall(r"\batomic\w*\(", code) == [] and "__hip_atomic" not in code and "asm" not in code and "pow(" not in code
    assert "iem_grad_atomic(" not in code and "iem_grad_wave_uniform(" not in code and "iem_last_arrival" not in code      # the helpers' float atomics stay unused
    # no other object's source knows of it
    for f in (iemlib.mu_source, iemlib.barrier_mu_source, iemlib.barrier_source, iemlib.search_source, iemlib.soc_source):
        assert "amu_" not in f()[0]


@pytest.mark.skipif(not os.path.exists(_HIPCC), reason="no hipcc")
def test_the_object_compiles_without_scratch(built, tmp_path):
    from infiniteexamodels.jl_amd import lib as iemlib
    src, _ = iemlib.amu_source()
    head = src.split("\n", 1)[0]
    hip = tmp_path / "a.hip"
    hip.write_text(src)
    p = subprocess.run([_HIPCC, "--genco", "--offload-arch=gfx950", *head[len("// iem-flags:"):].split(), "-Rpass-analysis=kernel-resource-usage",
                        "-o", str(tmp_path / "a.hsaco"), str(hip)], capture_output=True, text=True)
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
    assert L.iem_amu_create(N, N, C.byref(out)) == -4 and "null" in err()
    assert L.iem_amu_create(N, C.byref(iemlib.AmuOpts.defaults()), N) == -4 and "null" in err()
    assert L.iem_amu_destroy(N) == 0
    assert L.iem_amu_reset(N) == -4 and "null" in err()
    assert L.iem_amu_probe(N, *[N] * 14) == -4 and "null" in err()
    assert L.iem_amu_update(N, N, N, 0, N) == -4 and "null" in err()
    assert L.iem_amu_device(N, N) == -4 and "null" in err()
    assert L.iem_amu_state(N, N, N) == -4 and "null" in err()


def known(case, counts):
    """the restatement on one case, and the assertion that the branch of its label was taken"""
    blk, ab, ctl = aref.update(case["blk"], case["ab"], case["w"], case["probe"], counts, case["opts"], case["aopts"], case["force_fixed"],
                               np.arange(16, dtype=np.float64) + 1.0)
    iw, ia, want = mref.ints(blk), mref.ints(ab), case["want"]
    got = dict(status=int(iw[8]), mode=int(ia[aref.MODE]), k=int(iw[10]), changed=bool(iw[9] & 1), nrefs=int(ia[aref.NREFS]), mu=float(blk[0]),
               sigma=float(ab[aref.SIGMA]), to_fixed=int(ia[aref.TO_FIXED]), to_free=int(ia[aref.TO_FREE]), mu_max=float(ab[aref.MU_MAX]), refs_head=float(ab[aref.REF0]))
    for key, v in want.items():
        assert np.isclose(got[key], v, rtol=1e-12, atol=0.0) if isinstance(v, float) else got[key] == v, (case["label"], key, got[key], v)
    changed = got["changed"]
    assert changed == (bits(blk[0]) != bits(case["blk"][0])) and (ctl[11] == 0.0 and ctl[12] == 0.0) == changed
    assert np.array_equal(np.delete(ctl, [11, 12]), np.delete(np.arange(16) + 1.0, [11, 12])) and iw[11] == 1
    if changed:
        assert bits(blk[1]) == bits(np.maximum(np.float64(case["opts"]["tau_min"]), 1.0 - blk[0])) and bits(blk[2]) == bits(np.sqrt(blk[0]))
    else:
        assert bits(blk[:3]).tolist() == bits(case["blk"][:3]).tolist()
    if got["status"] != mref.ITERATING:
        assert bits(ab).tolist() == bits(case["ab"]).tolist(), case["label"]      # the own block stays
    return got


@pytest.mark.parametrize("counts", COUNTS)
@pytest.mark.parametrize("oracle", [aref.PROBING, aref.LOQO])
def test_every_branch_is_reached(oracle, counts, built):
    cases = aref.branch_cases(oracle, counts)
    seen = {c["label"]: known(c, counts) for c in cases}
    assert len(seen) == len(cases)      # the labels are distinct
    if counts[1] == 0:
        assert seen["nz = 0: mu_min"]["changed"] and not seen["nz = 0: mu stays"]["changed"]
        return
    need = ["converged", "the first update sets mu_max", "free, progress, the ring filling", "free, progress, a full ring: the oldest leaves", "free to fixed: no progress",
            "free to fixed: forced", "fixed, no decrease: mu unchanged", "fixed, one decrease", "fixed, several decreases", "fixed to free",
            "free: the oracle's mu is the block's"]
    need += (["unusable: a NaN product in the probe", "unusable: alpha_p is +0.0", "unusable: alpha_d is +0.0", "probing: unclamped", "probing: clamped at mu_min",
              "probing: clamped at mu_max", "probing: sigma capped by sigma_max"] if oracle == aref.PROBING else
             ["LOQO: unclamped, xi = 1/2", "LOQO: xi = 1, clamped at mu_min", "LOQO: xi = 0", "LOQO: xi = 0, clamped at mu_max"])
    assert set(need) <= set(seen), set(need) - set(seen)
    full = next(c for c in cases if c["label"].startswith("free, progress, a full ring"))
    _, ab, _ = aref.update(full["blk"], full["ab"], full["w"], full["probe"], counts, full["opts"], full["aopts"])
    assert ab[aref.REF0:aref.REF0 + 3].tolist() == [0.5, 0.3, 0.1] and bits(ab[aref.REF0 + 3]) == bits(0.02)      # E(0) of the hand-made words


@pytest.mark.parametrize("name", ["opf_7", "pandemic_20x3"])
@pytest.mark.parametrize("oracle", [aref.PROBING, aref.LOQO])
def test_fixed_mode_without_progress_is_the_monotone_rule(name, oracle, built):
    aopts = aref.options(oracle=oracle)
    for label, P, st, blk, opts, want in mref.branch_cases(name):
        counts = (P["B"]["counts"]["ncon"], P["B"]["counts"]["nz"])
        w = word_vector(P, st)
        ctl = np.arange(16, dtype=np.float64) + 1.0
        ab = aref.own_block(aopts, aref.FIXED, 1e300, (0.0,) * 4)      # no E(0) > 0 is progress against references of zero
        probe = np.array([1.0, 0.0, 1.0, 1.0]) if oracle == aref.PROBING else None
        ref, ctl_ref = mref.update(blk, w, counts, opts, ctl)
        got, ab2, ctl2 = aref.update(blk, ab, w, probe, counts, opts, aopts, False, ctl)
        assert bits(got).tolist() == bits(ref).tolist(), (label, got, ref)      # mu, tau, zeta, the errors, status, flag, decreases, updates
        assert bits(ctl2).tolist() == bits(ctl_ref).tolist()
        assert mref.ints(ab2)[aref.MODE] == aref.FIXED and mref.ints(ab2)[aref.TO_FREE] == 0


def test_equal_products_give_loqo_sigma_zero(built):
    """eight variables on exact lower bounds 0, x a power of two, z = 1/(4x): every product is 1/4 exactly, their sum 2"""
    n = 8
    x = 2.0 ** np.arange(-3, n - 3)
    none, off = np.full(n, np.inf), np.zeros(n, dtype=bool)
    e = np.zeros(0)
    B = dict(xl=np.zeros(n), xu=none, rl=e, ru=e, hasL=~off, hasU=off, gL=e.astype(bool), gU=e.astype(bool))
    st = (x, e, e, 0.25 / x, np.full(n, np.nan), e, e)
    p = mref.products(B, st)
    assert (p == 0.25).all() and len(p) == n
    w = aref.words(n, pmax=float(p.max()), pmin=float(p.min()), avg=0.25)
    assert w[9] == float(np.sum(p)) == 2.0
    opts, aopts = mref.options(), aref.options(oracle=aref.LOQO)
    blk, ab, _ = aref.update(mref.fresh_block(opts), aref.fresh_block(aopts), w, None, (0, n), opts, aopts)
    assert bits(ab[aref.SIGMA]) == bits(0.0) and bits(ab[aref.MU_ORACLE]) == bits(0.0) and blk[0] == aopts["mu_min"]
    assert mref.ints(ab)[aref.MODE] == aref.FREE and ab[aref.AVG] == 0.25


@pytest.mark.parametrize("name", ["opf_7", "farmer_5", "pandemic_20x3"])
def test_the_probe_at_zero_directions_sums_the_products(name, built):
    P = bref.barrier_point(name)
    B, st = P["B"], P["state"]
    n, m = len(st[0]), len(st[1])
    zero = (np.zeros(m), np.zeros(n), np.zeros(n), np.zeros(m), np.zeros(m))
    p, nan, ap, ad = aref.probe_words(B, st, np.zeros(n + m), zero, (1.0, 1.0))
    want = mref.products(B, st)
    assert bits(p).tolist() == bits(want).tolist() and nan == 0.0 and (ap, ad) == (1.0, 1.0) and len(p) == B["counts"]["nz"]
    # a NaN direction at a present bound is counted; at an absent bound it is not seen
    picks = [(int(np.flatnonzero(on)[0]), count) for on, count in ((B["hasL"], 1.0), (~B["hasL"], 0.0)) if on.any()]
    for i, count in picks:
        d = [a.copy() for a in zero]
        d[1][i] = np.nan
        assert aref.probe_words(B, st, np.zeros(n + m), tuple(d), (1.0, 1.0))[1] == count
