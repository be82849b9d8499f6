"""The barrier parameter object (iem_mu_*, csrc/iem_mu_device.h) and the three bindings on the MI355X.

BITWISE against the device's own iem_barrier_error (words 0–7 of iem_mu_error), against numpy (the extremes, the count) and against
tests/mu_reference.py (the whole block after iem_mu_update on every branch; a ladder of decreases from mu_init to the floor and 10⁴
log-uniform mu: the check of the device's sqrt).  Word 9, the sum of the products, carries the bits of mu_reference.product_sums —
the restatement in the DEVICE'S ORDER (barrier_reference.device_sum) on the object's own grid of info["workgroups"] workgroups; the
count of word 10 goes through the same column — and repeats bit for bit.  Bound calls given wrong host scalars write the bits of the
unbound calls given the block's; one captured iteration replays across a change of mu.

Shapes: opf_7 (two workgroups), quadrotor_100 (several workgroups: the last-arrival path; no bound at all), `maratos` (nz = 0, every
row an equality) and the two big shapes of barrier_reference.big_point, random bounds of every kind and a random interior state on
4096 workgroups of 256: quadrotor(27 000) (nvar + ncon = 1 080 000 > 2²⁰: the grid-stride loop runs a second trip, rows only) and
quadrotor(60 000) (nvar = 1 320 000 > 2²⁰: three trips, the second across the nvar seam — asserted and printed).  At the big shapes
every extreme slot of iem_mu_error (the four maxima, the minimum of word 8) is also planted at either side of the nvar seam, at
2²⁰ − 1, 2²⁰, the first entry of trip three and n − 1 in turn, and the −0.0 multiplier is counted there."""
import contextlib
import ctypes as C
import math
import types

import numpy as np
import pytest

import barrier_reference as bref
import mu_reference as mref
import soc_reference

pytestmark = pytest.mark.gpu
BIG = {"quadrotor_27000": 27_000, "quadrotor_60000": 60_000}
SHAPES = ["opf_7", "quadrotor_100", "maratos"] + list(BIG)
NAN = float("nan")
PAD = 5
WRONG_MU, WRONG_TAU = 123.0, 0.5


def T(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def H(t):
    return t.cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


_hip = []


def hip():
    """the HIP runtime of this process (the one torch loaded), for copies to and from the objects' own device memory"""
    if not _hip:
        path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
        rt = C.CDLL(path)
        rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        rt.hipMemcpy.restype = C.c_int
        _hip.append(rt)
    return _hip[0]


def peek(ptr, n=16):
    import torch
    torch.cuda.synchronize()
    out = np.empty(n)
    assert hip().hipMemcpy(out.ctypes.data, ptr, 8 * n, 2) == 0
    return out


def poke(ptr, a):
    import torch
    torch.cuda.synchronize()
    a = np.ascontiguousarray(a, dtype=np.float64)
    assert hip().hipMemcpy(ptr, a.ctypes.data, a.nbytes, 1) == 0


def big_point(supports=27_000):
    """barrier_reference.big_point: quadrotor(supports) with bounds and a state of the tests' own, built once per size"""
    return bref.big_point(supports)


def point(name):
    return big_point(BIG[name]) if name in BIG else soc_reference.point(name)


def big_facts(name, S):
    """the grid and the trips of a big shape, asserted instead of trusted, and printed"""
    n_wg = S.bar.info["workgroups"]
    trips = bref.trips(S.nvar, S.n, n_wg)
    print(f"{name}: n {S.n}, workgroups {n_wg}, trips {len(trips)}, (variables, rows) per trip {trips}")
    assert n_wg == min(-(-S.n // 256), 4096) == 4096
    if name == "quadrotor_60000":
        assert (S.nvar, S.ncon, S.n) == (1_320_000, 1_080_000, 2_400_000) and S.nvar > 2 ** 20
        assert len(trips) == 3 and trips[0][1] == 0 and trips[1][0] > 0 and trips[1][1] > 0 and trips[2][0] == 0 and trips[2][1] > 0
    else:
        assert S.n == 1_080_000 and S.nvar < 2 ** 20 < S.n and len(trips) == 2 and trips[1][0] == 0 and trips[1][1] > 0


@contextlib.contextmanager
def objects(P, **mu_opts):
    """the model handle, a BarrierLayer on P's bounds, a BarrierParameter, and P's state, r, c on the device"""
    from infiniteexamodels.jl_amd.barrier import BarrierLayer, BarrierParameter
    from infiniteexamodels.jl_amd.model import ExaModel
    gm = ExaModel(P["core"], device=0, blob=P["blob"]) if P["blob"] is not None else ExaModel(P["core"], device=0)
    try:
        with BarrierLayer(gm, relax=bref.RELAX, bounds=(P["lvar"], P["uvar"], P["lcon"], P["ucon"])) as bar, BarrierParameter(bar, **mu_opts) as par:
            B = P["B"]
            assert all(bar.info[k] == v for k, v in B["counts"].items())
            S = types.SimpleNamespace(gm=gm, bar=bar, par=par, P=P, B=B, counts=(B["counts"]["ncon"], B["counts"]["nz"]), nvar=bar.nvar, ncon=bar.ncon, n=bar.n,
                                      st=tuple(T(a) for a in P["state"]), r=T(P["r"]), c=T(P["c"]), blk=par.device())
            yield S
    finally:
        gm.close()


def words(S, st=None, r=None, c=None):
    """iem_mu_error into a NaN-poisoned buffer: the twelve words on the host, the padding checked"""
    import torch
    buf = torch.full((12 + PAD,), NAN, dtype=torch.float64, device="cuda")
    S.par.error(st if st is not None else S.st, r if r is not None else S.r, c if c is not None else S.c, out=buf[:12])
    h = H(buf)
    assert np.isnan(h[12:]).all(), "padding touched"
    return h[:12]


@pytest.mark.parametrize("name", SHAPES)
def test_error_words(name, built):
    import torch
    P = point(name)
    with objects(P) as S:
        B, st_h = S.B, P["state"]
        w = words(S)
        e8 = H(S.bar.error(S.st, S.r, S.c, 0.0, out=torch.full((8,), NAN, dtype=torch.float64, device="cuda")))
        assert same_bits(w[:8], e8), (w[:8], e8)
        head, _, w8, w10, p = mref.error_words(B, st_h, P["r"], P["c"])
        assert same_bits(w[:4], head)
        n_wg = S.bar.info["workgroups"]
        assert n_wg == min(-(-S.n // 256), 4096)
        if name in BIG:
            big_facts(name, S)
        w9, c10 = mref.product_sums(B, st_h, n_wg)
        print(name, "workgroups", n_wg, "nz", S.counts[1], "w8", w[8], "w9", repr(w[9]), "device order", repr(float(w9)), "fsum", math.fsum(p), "w10", w[10])
        assert same_bits(w[8], w8) and same_bits(w[10], w10) and w10 == 0.0 and same_bits(w[11], 0.0) and same_bits(c10, w10)
        assert same_bits(w[9], w9), (w[9], w9)
        assert same_bits(words(S), w)      # the same bits again: the sums have one order
        if S.counts[1] == 0:
            assert w[8] == np.inf and w[3] == 0.0 and same_bits(w[9], 0.0)
            return
        # one multiplier NaN, one product negative: counted, kept out of the minimum
        where = [(3, B["hasL"]), (4, B["hasU"]), (5, B["gL"]), (6, B["gU"])]
        k, on = next((k, on) for k, on in where if on.any())
        i = int(np.flatnonzero(on)[-1])
        for value in (NAN, -1.0):
            bad = [a.copy() for a in st_h]
            bad[k][i] = value
            _, _, b8, b10, bp = mref.error_words(B, tuple(bad), P["r"], P["c"])
            st = list(S.st)
            st[k] = T(bad[k])
            wb = words(S, st=tuple(st))
            assert b10 == 1.0 and same_bits(wb[10], 1.0) and same_bits(wb[8], b8), (value, wb)
            assert np.isnan(wb[3]) if value != value else same_bits(wb[3], np.abs(bp).max())
            b9, c10 = mref.product_sums(B, tuple(bad), n_wg)
            assert same_bits(wb[9], b9) if value == value else np.isnan(wb[9]) and np.isnan(b9)
            assert same_bits(c10, 1.0)
        # −0.0 is not >= +0.0 on the bit patterns: a zero multiplier under a negative zero
        bad = [a.copy() for a in st_h]
        bad[k][i] = -0.0
        st = list(S.st)
        st[k] = T(bad[k])
        wb = words(S, st=tuple(st))
        assert same_bits(wb[10], 1.0)


@pytest.mark.parametrize("name", list(BIG))
def test_big_extremes_on_later_trips(name, built):
    """the four maxima and the minimum of word 8 with their deciding value planted at each seam position in turn (module docstring):
    the slot carries the bits numpy gives for the planted entry, which beats the rest of the state; and a −0.0 multiplier there is
    counted in word 10"""
    P = point(name)
    with objects(P) as S:
        B, st_h, r_h, c_h = S.B, P["state"], P["r"], P["c"]
        big_facts(name, S)
        n = S.nvar
        no_x, no_s = np.zeros(S.nvar, dtype=bool), np.zeros(S.ncon, dtype=bool)
        masks = {"variable": np.concatenate([~no_x, no_s]), "row": np.concatenate([no_x, ~no_s]), "inequality row": np.concatenate([no_x, ~B["eq"]]),
                 "lower": np.concatenate([B["hasL"], B["gL"]])}

        def planted(kind):
            out, seen = [], set()
            for label, i in bref.seam_positions(S.nvar, S.n, S.bar.info["workgroups"]).items():
                k = bref.nearest(masks[kind], i)
                assert masks[kind][k]
                if k not in seen:
                    seen.add(k)
                    out.append((f"{label} -> {k}", k))
            return out
        base = words(S)
        head, _, w8, w10, _ = mref.error_words(B, st_h, r_h, c_h)
        assert same_bits(base[:4], head) and same_bits(base[8], w8) and w10 == 0.0
        dev_vec = {"r": S.r, "y": S.st[2], "c": S.c}
        for slot, what, kind, value in ((0, "r", "variable", 1e30), (1, "y", "inequality row", 1e30), (2, "c", "row", 1e30), (3, "z", "lower", 1e30), (8, "z", "lower", 1e-30),
                                        (10, "z", "lower", -0.0)):
            for label, i in planted(kind):
                iv, ir = (np.array([i]), np.array([], dtype=np.int64)) if i < n else (np.array([], dtype=np.int64), np.array([i - n]))
                B1, st1 = bref.cut(B, iv, ir), [a.copy() for a in bref.cut_state(st_h, iv, ir)]
                r1, c1 = r_h[iv].copy(), c_h[ir].copy()
                j = i if i < n else i - n
                vec = dev_vec[what] if what != "z" else (S.st[3] if i < n else S.st[5])
                host_vec = {"r": r1, "y": st1[2], "c": c1, "z": st1[3] if i < n else st1[5]}[what]
                old = float(vec[j])
                vec[j] = value
                host_vec[0] = value
                got = words(S)
                h1, _, m1, bad1, _ = mref.error_words(B1, tuple(st1), r1 if len(iv) else np.zeros(0), c1)
                want_head = np.maximum(base[:4], np.where(np.isnan(h1), 0.0, h1))
                print(f"{name} word {slot} planted ({what} = {value}) at {label}: head {got[:4].tolist()}, w8 {got[8]}, w10 {got[10]}")
                assert same_bits(got[:4], want_head) and same_bits(got[8], min(float(base[8]), m1)) and same_bits(got[10], bad1), (slot, label, got)
                if slot < 4:
                    assert h1[slot] > base[slot]
                elif slot == 8:
                    assert m1 < base[8]
                else:
                    assert bad1 == 1.0 and same_bits(got[8], base[8])      # −0.0 is not >= +0.0 on the bit patterns: counted, kept out of the minimum
                vec[j] = old
        assert same_bits(words(S), base)


def pattern_search(S, fs):
    """a search whose control block and filter hold a recognisable pattern: (ctl pointer, filter pointer, ctl, filter)"""
    ctl_ptr, flt_ptr = fs.device()
    ctl = np.arange(16, dtype=np.float64) + 1.5
    ctl.view(np.int64)[11], ctl.view(np.int64)[12] = 3, 1
    flt = np.arange(2 * fs.opts["filter_capacity"], dtype=np.float64) + 0.25
    poke(ctl_ptr, ctl)
    poke(flt_ptr, flt)
    return ctl_ptr, flt_ptr, ctl, flt


@pytest.mark.parametrize("name", ["opf_7", "pandemic_20x3"])
def test_update_branches(name, built):
    """the whole block is the restatement's on every branch of tests/test_mu.py (b), from the DEVICE's twelve words; a search's words
    11, 12 are cleared exactly when mu moved, its other fourteen words and its filter never"""
    from infiniteexamodels.jl_amd.barrier import BarrierParameter, FilterSearch
    P0 = bref.barrier_point(name)
    seen = {}
    with objects(P0) as S, FilterSearch(S.bar) as fs:
        for label, P, st_h, blk0, opts, want in mref.branch_cases(name):
            over = {k: v for k, v in opts.items() if v != mref.options()[k]}
            with BarrierParameter(S.bar, **over) as par:
                S.par, ptr = par, par.device()
                par.reset(float(blk0[0]))
                before = peek(ptr)
                assert same_bits(before, blk0), (label, before, blk0)
                st, r, c = tuple(T(a) for a in st_h), T(P["r"]), T(P["c"])
                w = words(S, st, r, c)
                ctl_ptr, flt_ptr, ctl, flt = pattern_search(S, fs)
                wd = T(w)
                par.update(wd, search=fs)
                blk = peek(ptr)
                ref, ctl_ref = mref.update(before, w, S.counts, opts, ctl)
                iw = mref.ints(blk)
                print(name, label, "mu", blk[0], "tau", blk[1], "E0", blk[3], "Emu", blk[4], "status", iw[8], "flags", iw[9], "decreases", iw[10])
                assert same_bits(blk, ref), (label, blk, ref)
                assert same_bits(peek(ctl_ptr), ctl_ref) and same_bits(peek(flt_ptr, len(flt)), flt), label
                assert (iw[9] & 1) == int(iw[10] > 0) and same_bits(ctl_ref[11:13], [0.0, 0.0]) == bool(iw[10] > 0)
                s = par.state()
                assert same_bits([s[k] for k in ("mu", "tau", "zeta", "e0", "e_mu", "e_d", "e_p", "e_c0")], blk[:8])
                assert (s["status"], s["flags"], s["decreases"], s["updates"]) == tuple(iw[8:12]) and s["changed"] == bool(iw[9] & 1)
                # without a search: the same block, the search untouched
                par.reset(float(blk0[0]))
                par.update(wd)
                assert same_bits(peek(ptr), ref) and same_bits(peek(ctl_ptr), ctl_ref)
                seen[label] = (int(iw[10]), int(iw[8]))
                if want == ">=3":
                    assert iw[10] >= 3
                elif want is not None:
                    assert iw[10] == want
        assert seen["converged"][1] == mref.CONVERGED and seen["a NaN multiplier"][1] == mref.UNUSABLE and seen["a negative product"][1] == mref.UNUSABLE
        assert seen["stop at the floor"][0] >= 1 and seen["one decrease"] == (1, mref.ITERATING) and seen["far from the path"] == (0, mref.ITERATING)


def test_the_ladder_and_the_square_root(built):
    """From hand-made words (only complementarity in the error, products all 1e-30): ONE update walks from mu_init down to the floor;
    then 10⁴ log-uniform mu in [1e-12, 1], each through reset (zeta = sqrt(mu0)) and an update that decreases until the floor — words
    0–2 and the counters are the restatement's, bit for bit: the device's sqrt is the correctly rounded one."""
    import torch
    P = bref.barrier_point("opf_7")
    with objects(P) as S:
        w = np.zeros(12)
        w[3] = w[8] = 1e-30
        w[4] = w[5] = 1.0
        wd = T(w)
        # the actual ladder of the defaults, stopped by the default floor
        opts = mref.options(tol=1e-40)
        from infiniteexamodels.jl_amd.barrier import BarrierParameter
        with BarrierParameter(S.bar, tol=1e-40) as par:
            assert par.opts["mu_floor"] == 1e-11
            before = peek(par.device())
            par.update(wd)
            blk = peek(par.device())
            ref, _ = mref.update(before, w, S.counts, opts)
            print("ladder: decreases", mref.ints(blk)[10], "mu", blk[0], "tau", blk[1], "zeta", blk[2])
            assert same_bits(blk, ref) and blk[0] == 1e-11 and mref.ints(blk)[10] >= 5
        o = dict(tol=1e-40, mu_floor=1e-25)
        opts = mref.options(**o)
        mus = 10.0 ** np.random.default_rng(5).uniform(-12.0, 0.0, 10_000)
        with BarrierParameter(S.bar, **o) as par:
            ptr = par.device()
            got = torch.empty((len(mus), 16), dtype=torch.float64, device="cuda")
            base = got.data_ptr()
            rt = hip()
            torch.cuda.synchronize()
            for i, mu0 in enumerate(mus):
                par.reset(float(mu0))
                par.update(wd)
                assert rt.hipMemcpy(base + 128 * i, ptr, 128, 3) == 0      # device to device, behind the stream's work
            got = H(got)
        zero = np.zeros(16)
        worst = 0
        for i, mu0 in enumerate(mus):
            start = mref.reset(zero, opts, mu0)
            ref, _ = mref.update(start, w, S.counts, opts)
            assert same_bits(got[i], ref), (i, mu0, got[i], ref)
            worst = max(worst, int(mref.ints(ref)[10]))
        print("10^4 mu: most decreases in one update", worst)
        assert worst >= 4


def _eight(S, fs, soc, mu, tau, data):
    """the eight kernels that read mu, each from the same inputs: every output (and the search's block) on the host"""
    import torch
    out = {}
    st = tuple(t.clone() for t in S.st)
    sol, dirs0, rhs1, ct, s_t = data["sol"], data["dirs"], data["rhs"], data["ct"], data["st"]
    nanv = lambda k: torch.full((k,), NAN, dtype=torch.float64, device="cuda")
    sigma, dcon, rhs = S.bar.terms(st, S.r, S.c, mu, out=(nanv(S.nvar), nanv(S.ncon), nanv(S.n)))
    out["terms"] = [H(sigma), H(dcon), H(rhs)]
    dirs, alpha = S.bar.step(st, sol, mu, tau, out=tuple(nanv(k) for k in (S.ncon, S.nvar, S.nvar, S.ncon, S.ncon)), alpha=nanv(2))
    out["step"] = [H(d) for d in dirs] + [H(alpha)]
    S.bar.update(st, sol, dirs0, T([0.5, 0.25]), mu, kappa_sigma=1.0)      # kappa_sigma = 1: the safeguard leaves z = mu/gap, so mu shows
    out["update"] = [H(t) for t in st]
    out["error"] = [H(S.bar.error(S.st, S.r, S.c, mu, out=nanv(8)))]
    ctl_ptr, flt_ptr = fs.device()
    poke(ctl_ptr, data["ctl_unusable"])
    fs.begin(S.st, data["g"], sol, dirs0[0], T([1.25]), T(data["err8"]), T([0.75, 0.5]), mu)
    out["begin"] = [peek(ctl_ptr)]
    a = T([NAN, 0.5])
    fs.accept(T([1.5]), T([0.3, -7.0]), mu, a)
    out["accept"] = [peek(ctl_ptr), H(a)]
    poke(ctl_ptr, data["ctl_soc"])
    out["soc_rhs"] = [H(soc.rhs(S.st, S.c, ct, s_t, rhs1, mu, out=nanv(S.n)))]
    a = T([NAN, NAN])
    soc.accept(T([1.5]), T([0.3, -7.0]), T([0.5, 0.25]), mu, a)
    out["soc_accept"] = [peek(ctl_ptr), H(a)]
    return out


def _equal(a, b):
    return {k: all(same_bits(x, y) for x, y in zip(a[k], b[k])) for k in a}


def test_binding(built):
    """each of the eight kernels, bound and given mu = 123, tau = 0.5, writes the bits of the unbound call given the block's mu and
    tau; unbound again the host arguments rule; a parameter of another barrier object is refused"""
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.barrier import BarrierLayer, BarrierParameter, FilterSearch, SecondOrderCorrection
    P = bref.barrier_point("opf_7")
    with objects(P, mu_init=0.037) as S, FilterSearch(S.bar) as fs, SecondOrderCorrection(fs) as soc:
        B = S.B
        assert B["counts"]["n_ineq"] > 0 and B["counts"]["nz"] > 0
        rng = np.random.default_rng(11)
        blk = peek(S.blk)
        mu_b, tau_b = float(blk[0]), float(blk[1])
        assert (mu_b, tau_b) == (0.037, 0.99)
        ine = ~B["eq"]
        rnd = lambda k, on=None: np.where(on, rng.standard_normal(k), NAN) if on is not None else rng.standard_normal(k)
        ctl_soc = np.zeros(16)
        ctl_soc[:9] = [0.75, 0.75, 2.0, 0.5, -1.0, 1e-4, 1e4, NAN, 0.6]
        ctl_soc.view(np.int64)[9:15] = [0, 1, 0, 1, 1, 0]      # SEARCHING, one trial, flags bit 0, the correction ACTIVE, no round yet
        ctl_soc[15] = 0.75
        ctl_un = np.zeros(16)
        ctl_un.view(np.int64)[9] = 4
        data = dict(sol=T(rnd(S.n)), dirs=(T(rnd(S.ncon, ine)), T(rnd(S.nvar)), T(rnd(S.nvar)), T(rnd(S.ncon, ine)), T(rnd(S.ncon, ine))), rhs=T(rnd(S.n)),
                    ct=T(rnd(S.ncon)), st=T(np.where(ine, P["state"][1] + 0.01 * rng.standard_normal(S.ncon), NAN)), g=T(rnd(S.nvar)),
                    err8=np.array([0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.4, -3.0]), ctl_soc=ctl_soc, ctl_unusable=ctl_un)
        want = _eight(S, fs, soc, mu_b, tau_b, data)
        wrong = _eight(S, fs, soc, WRONG_MU, WRONG_TAU, data)
        differs = _equal(want, wrong)
        assert not any(differs.values()), differs      # the scalars matter to every one of the eight
        S.bar.bind_mu(S.par); fs.bind_mu(S.par); soc.bind_mu(S.par)
        bound = _eight(S, fs, soc, WRONG_MU, WRONG_TAU, data)
        assert all(_equal(bound, want).values()), _equal(bound, want)
        assert all(_equal(_eight(S, fs, soc, -1.0, 7.0, data), want).values())      # the range checks are the block's business now
        # one object bound: only its kernels follow the block
        fs.bind_mu(None); soc.bind_mu(None)
        mixed = _equal(_eight(S, fs, soc, WRONG_MU, WRONG_TAU, data), want)
        assert mixed == dict(terms=True, step=True, update=True, error=True, begin=False, accept=False, soc_rhs=False, soc_accept=False), mixed
        S.bar.bind_mu(None)
        assert all(_equal(_eight(S, fs, soc, WRONG_MU, WRONG_TAU, data), wrong).values())
        with pytest.raises(iemlib.IemError, match="mu"):
            S.bar.terms(S.st, S.r, S.c, -1.0)
        with BarrierLayer(S.gm, relax=bref.RELAX) as bar2, BarrierParameter(bar2) as par2:
            for obj in (S.bar, fs, soc):
                with pytest.raises(iemlib.IemError, match="another barrier object"):
                    obj.bind_mu(par2)
            with FilterSearch(bar2) as fs2:
                with pytest.raises(iemlib.IemError, match="another barrier object"):
                    S.par.update(T(np.zeros(12)), search=fs2)
        assert all(_equal(_eight(S, fs, soc, mu_b, tau_b, data), want).values())      # a refused bind binds nothing


def _iteration(S, fs, bufs, par=None, mu=None, tau=None):
    """mu_error, mu_update(search) — unbound: barrier_error(0) —, terms, step on the given sol, begin, one rung, update"""
    b, gm = S.bar, S.gm
    if par is not None:
        par.error(b_state(bufs), bufs["r"], bufs["c"], out=bufs["w"])
        par.update(bufs["w"], search=fs)
    else:
        b.error(b_state(bufs), bufs["r"], bufs["c"], 0.0, out=bufs["w"][:8])
    mu, tau = (WRONG_MU, WRONG_TAU) if par is not None else (mu, tau)
    st = b_state(bufs)
    b.terms(st, bufs["r"], bufs["c"], mu, out=(bufs["sigma"], bufs["dcon"], bufs["rhs"]))
    b.step(st, bufs["sol"], mu, tau, out=bufs["dirs"], alpha=bufs["alpha"])
    fs.begin(st, bufs["g"], bufs["sol"], bufs["dirs"][0], bufs["f"], bufs["w"][:8], bufs["alpha"], mu)
    fs.trial(st, bufs["sol"], bufs["dirs"][0], bufs["xt"], bufs["s_t"])
    gm.obj_device(bufs["xt"], out=bufs["ft"])
    gm.cons(bufs["xt"], bufs["ct"])
    b.merit(bufs["xt"], bufs["s_t"], bufs["ct"], out=bufs["mt"])
    fs.accept(bufs["ft"], bufs["mt"], mu, bufs["alpha"])
    b.update(st, bufs["sol"], bufs["dirs"], bufs["alpha"], mu)


def b_state(bufs):
    return bufs["state"]


def test_one_graph_across_two_barrier_problems(built):
    """ONE captured iteration replayed from a state that leaves mu alone and from one near the central path that lowers it: every
    buffer is bitwise the eager UNBOUND sequence called with the restatement's mu and tau.  (The direction is random and the
    "objective at the current point" is 1e12, far above any value at a trial point, so from the first state the one rung accepts and
    the update moves.  The second state has a made-up feasible c: mu moves, the filter and theta_max start again, and the rung may be
    rejected on the real c(xt) — then the update is seen to move nothing, in both sequences.)"""
    import torch
    from infiniteexamodels.jl_amd.barrier import FilterSearch
    name = "opf_7"
    P = bref.barrier_point(name)
    far = (P, P["state"])
    near = next((Q, st) for label, Q, st, _, _, _ in mref.branch_cases(name) if label == "several decreases")
    with objects(P) as S, FilterSearch(S.bar) as fs:
        rng = np.random.default_rng(21)
        nanv = lambda k: torch.full((k,), NAN, dtype=torch.float64, device="cuda")
        sol_h, g_h = 1e-3 * rng.standard_normal(S.n), rng.standard_normal(S.nvar)
        bufs = dict(state=tuple(nanv(len(a)) for a in P["state"]), r=nanv(S.nvar), c=nanv(S.ncon), w=nanv(12), sigma=nanv(S.nvar), dcon=nanv(S.ncon), rhs=nanv(S.n),
                    sol=T(sol_h), g=T(g_h), dirs=tuple(nanv(k) for k in (S.ncon, S.nvar, S.nvar, S.ncon, S.ncon)), alpha=nanv(2), f=T([1e12]), xt=nanv(S.nvar),
                    s_t=nanv(S.ncon), ct=nanv(S.ncon), ft=nanv(1), mt=nanv(2))
        ctl_ptr, flt_ptr = fs.device()
        cap = fs.opts["filter_capacity"]
        flt0 = np.zeros(2 * cap)
        flt0[:2] = [1e300, 1e300]      # an entry that bars no trial point: the filter is seen to be emptied, or kept
        ctl0 = np.zeros(16)
        ctl0.view(np.int64)[9], ctl0.view(np.int64)[11], ctl0.view(np.int64)[12] = 4, 1, 1
        ctl0[5], ctl0[6] = 1e-4, 1e300      # theta_min, theta_max of an earlier search (flag bit 0): no ceiling on theta while mu stays

        def load(case, blk):
            Q, st_h = case
            for t, a in zip(bufs["state"], st_h):
                t.copy_(T(a))
            bufs["r"].copy_(T(Q["r"])); bufs["c"].copy_(T(Q["c"]))
            for k in ("w", "sigma", "dcon", "rhs", "alpha", "xt", "s_t", "ct", "ft", "mt"):
                bufs[k].fill_(NAN)
            for t in bufs["dirs"]:
                t.fill_(NAN)
            poke(ctl_ptr, ctl0); poke(flt_ptr, flt0); poke(S.blk, blk)

        def results():
            flat = [H(t) for t in bufs["state"]] + [H(bufs[k]) for k in ("w", "sigma", "dcon", "rhs", "alpha", "xt", "s_t", "ct", "ft", "mt")] + [H(t) for t in bufs["dirs"]]
            return flat, peek(ctl_ptr), peek(flt_ptr, 2 * cap)
        opts = mref.options()
        blk0 = mref.fresh_block(opts)
        # the eager unbound sequences, with the restatement's mu and tau
        expected = {}
        for label, case in (("far", far), ("near", near)):
            load(case, blk0)
            w12 = words(S, bufs["state"], bufs["r"], bufs["c"])
            ref_blk, _ = mref.update(blk0, w12, S.counts, opts)
            moved = bool(mref.ints(ref_blk)[9] & 1)
            if moved:
                c2 = ctl0.copy()
                c2[11] = c2[12] = 0.0
                poke(ctl_ptr, c2)      # the host's fs.reset()
            _iteration(S, fs, bufs, None, float(ref_blk[0]), float(ref_blk[1]))
            flat, ctl, flt = results()
            flat[7] = np.concatenate([flat[7][:8], w12[8:]])      # (the unbound sequence has no words 8–11)
            expected[label] = (flat, ctl, flt, ref_blk, moved)
            print(label, "mu", ref_blk[0], "tau", ref_blk[1], "decreases", mref.ints(ref_blk)[10], "alpha", flat[11], "status", ctl.view(np.int64)[9])
        assert not expected["far"][4] and expected["near"][4] and expected["near"][3][0] < 0.1
        assert not same_bits(expected["far"][0][0], P["state"][0])      # the far iteration took a step
        # captured once, bound, with wrong host scalars
        S.bar.bind_mu(S.par); fs.bind_mu(S.par)
        load(far, blk0)
        _iteration(S, fs, bufs, S.par)      # (a warm run outside the capture)
        load(far, blk0)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            _iteration(S, fs, bufs, S.par)
        S.gm._sync_stream()
        for label, case in (("far", far), ("near", near), ("far", far)):
            load(case, blk0)
            g.replay()
            torch.cuda.synchronize()
            flat, ctl, flt = results()
            want = expected[label]
            for k, (a, b) in enumerate(zip(flat, want[0])):
                assert same_bits(a, b), (label, k)
            assert same_bits(ctl, want[1]) and same_bits(flt, want[2]), label
            assert same_bits(peek(S.blk), want[3]), label
        fs.bind_mu(None); S.bar.bind_mu(None)


def test_refusals(built):
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.barrier import BarrierParameter
    P = bref.barrier_point("opf_7")
    with objects(P) as S:
        L, b = S.bar._handle()
        err = lambda: L.iem_last_error().decode()
        out = C.c_void_p()
        inf = float("inf")
        for bad, word in ((dict(mu_init=0.0), "mu_init"), (dict(mu_init=-1.0), "mu_init"), (dict(kappa_mu=0.0), "kappa_mu"), (dict(kappa_mu=1.0), "kappa_mu"),
                          (dict(kappa_eps=0.0), "kappa_eps"), (dict(tau_min=0.0), "tau_min"), (dict(tau_min=1.0), "tau_min"), (dict(tol=0.0), "tol"),
                          (dict(mu_floor=-1e-9), "mu_floor"), (dict(s_max=0.0), "s_max"), (dict(s_max=inf), "finite"), (dict(mu_init=NAN), "finite"),
                          (dict(tol=inf), "finite"), (dict(kappa_eps=NAN), "finite")):
            o = iemlib.MuOpts.defaults(**bad)
            assert L.iem_mu_create(b, C.byref(o), C.byref(out)) == -4 and word in err(), bad
        o = iemlib.MuOpts.defaults(); o.struct_size = 4
        assert L.iem_mu_create(b, C.byref(o), C.byref(out)) == -4 and "struct_size" in err()
        assert L.iem_mu_create(None, None, C.byref(out)) == -4 and L.iem_mu_create(b, None, None) == -4 and "null" in err()
        raw = C.c_void_p()
        iemlib.check(L.iem_mu_create(b, None, C.byref(raw)))      # NULL options: the defaults
        assert same_bits(peek(_block(L, raw)), mref.fresh_block(mref.options()))
        before = peek(_block(L, raw))
        for mu0 in (0.0, -0.1, NAN, inf):
            assert L.iem_mu_reset(raw, mu0) == -4 and "mu0" in err()
        assert L.iem_mu_reset(None, 0.1) == -4
        pw = C.c_void_p(S.r.data_ptr())
        ptrs = [C.c_void_p(t.data_ptr()) for t in S.st] + [C.c_void_p(S.r.data_ptr()), C.c_void_p(S.c.data_ptr()), pw]
        for k in range(len(ptrs)):
            a = list(ptrs); a[k] = None
            assert L.iem_mu_error(raw, *a) == -4 and "null" in err(), k
        assert L.iem_mu_update(raw, None, None) == -4 and L.iem_mu_update(None, pw, None) == -4
        short = iemlib.MuState(); short.struct_size = 0
        assert L.iem_mu_state(raw, C.byref(short)) == -4 and "struct_size" in err()
        v = iemlib.MuState(); v.struct_size = 24; v.zeta = -5.0
        iemlib.check(L.iem_mu_state(raw, C.byref(v)))
        assert (v.mu, v.tau, v.zeta, v.struct_size) == (0.1, 0.99, -5.0, 24)      # a short struct receives its head only
        assert same_bits(peek(_block(L, raw)), before)      # a refused call does no device work
        iemlib.check(L.iem_mu_destroy(raw))
        assert L.iem_mu_destroy(None) == 0
        with pytest.raises(TypeError):
            BarrierParameter(S.bar, kappa=1.0)
        S.par.reset(0.25)
        s = S.par.state()
        assert (s["mu"], s["tau"], s["zeta"], s["status_name"], s["updates"]) == (0.25, 0.99, 0.5, "iterating", 0)
    with pytest.raises(iemlib.IemError, match="closed"):
        S.par.reset()


def _block(L, raw):
    p = C.c_void_p()
    assert L.iem_mu_device(raw, C.byref(p)) == 0
    return p.value


@pytest.mark.parametrize("name,want", [("rosenbrock", 306.4999755050365), ("ode_5x5", -12.784599900757165)])
def test_the_loop_with_mu_on_the_device(name, want, built):
    """tests/mu_loop.py with the parameter on the device and with the restatement on the host: bitwise the same x after every
    iteration (so the same count — printed; it is the reference here), the optimum and the error of
    tests/test_gpu_search.py::test_the_pieces_make_an_algorithm, no failed search."""
    import cases
    import mu_loop
    from infiniteexamodels.jl_amd import transcribe
    from infiniteexamodels.jl_amd.model import ExaModel
    core = transcribe.exa_core(cases.rosenbrock()[0]) if name == "rosenbrock" else cases.build_core(name)
    gm = ExaModel(core, device=0)
    try:
        res = {flag: mu_loop.solve(gm, device_mu=flag, tol=1e-8) for flag in (True, False)}
        for flag, r in res.items():
            print(name, "device_mu", flag, "iterations", r["iterations"], "objective", repr(r["objective"]), "error", r["error"], "mu", r["mu"], "decreases", r["decreases"],
                  "searches", r["statuses"])
            assert r["failed"] == 0 and set(r["statuses"]) <= {"accepted_f", "accepted_h"}, r["statuses"]
            assert r["status"] == mref.CONVERGED and r["error"] <= 1e-8 and abs(r["objective"] - want) <= 1e-6
        a, b = res[True], res[False]
        assert a["iterations"] == b["iterations"] and len(a["iterates"]) == len(b["iterates"]) == a["iterations"]
        for k, (xa, xb) in enumerate(zip(a["iterates"], b["iterates"])):
            assert same_bits(xa, xb), k
        assert same_bits(a["mu"], b["mu"]) and a["decreases"] == b["decreases"] and a["decreases"] >= 3
    finally:
        gm.close()
