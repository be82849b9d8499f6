"""The restoration phase's barrier parameter (iem_rmu_*, csrc/iem_rmu_device.h) and the bound restoration (iem_resto_bind_mu) on the
MI355X.

(a) iem_rmu_error on every model of tests/test_gpu_resto.py and on the two big shapes (4096 workgroups, two and three trips of the
stride loop): words 0–7 bitwise iem_resto_error(0, zeta_0) ON THE DEVICE and bitwise tests/rmu_reference.py in the device's order (the
sum of logs within barrier_reference.sum_bound, for the reason tests/test_gpu_resto.py gives); each candidate's two maxima bitwise
words 0 and 1 of an UNBOUND iem_resto_error(mu_k, zeta_k) on the device; words 8–10 bitwise the reference; extremes planted at entry 0,
nvar − 1, the first row, n − 1 and both sides of entry 4096·256 — each maximum's, a product below the minimum, a NaN, and a
reference point moved so far that the zeta term decides every candidate's maximum, once with r cancelling it at zeta_0 so that the
extreme sits in the later candidates; NaN poison wherever nothing may be read.
(b) every bound iem_resto_* kernel against the unbound call with the block's values as host doubles, garbage in the ignored host
arguments: every output vector, step length and block bit for bit; resto_check with and without a par_orig.
(c) every branch of enter, update and trigger on live objects, both blocks word for word against the reference (alpha_min within 4
ulp: the device's pow need not carry numpy's last bit; every decision exactly); the inner filter emptied exactly when mu moved; the
restoration block bitwise iem_mu_reset on a second object.
(d) one restoration iteration, bound, captured once and replayed at two states whose updates differ (no decrease, two decreases):
each replay bitwise the eager unbound sequence with the host's values.
(e) tests/rmu_loop.py: rule, STATIONARY exit and trigger on the device against the same words read back and rmu_reference deciding
on the host — bitwise the same iterates on wb_eq, wb_ineq and the classical model.
(f) the refusals."""
import contextlib
import ctypes as C
import math

import numpy as np
import pytest

import barrier_reference as bref
import mu_reference as mref
import resto_reference as rref
import rmu_reference as qref
import search_reference as sref
from barrier_reference import KAPPA, TAU
from test_gpu_barrier import BIG, big_facts
from test_gpu_resto import MODELS, layer, logs_within
from test_gpu_search import NAN, _p, dev, hip, host, nan, same_bits

pytestmark = pytest.mark.gpu
DELTA_C = 1e-10
GARBAGE = dict(mu=-1.0, tau=NAN, zeta=-3.0)      # what an unbound call refuses: a bound call must not look at them


class Rmu:
    """the raw iem_rmu object of a tests/test_gpu_resto.py Resto: create / destroy, the own block and the restoration block read and
    written through hipMemcpy"""

    def __init__(self, S, z, orig=None, **opts):
        from infiniteexamodels.jl_amd import lib as iemlib
        self.S, self.z, self.opts = S, z, dict(qref.OPTS, **opts)
        o = iemlib.RmuOpts.defaults(**opts)
        self.rp = C.c_void_p()
        S.check(S.L.iem_rmu_create(z.z, orig, C.byref(o), C.byref(self.rp)))
        blk, par, mblk = C.c_void_p(), C.c_void_p(), C.c_void_p()
        S.check(S.L.iem_rmu_device(self.rp, C.byref(blk)))
        S.check(S.L.iem_rmu_mu(self.rp, C.byref(par)))
        S.check(S.L.iem_mu_device(par, C.byref(mblk)))
        self.d_own, self.par, self.d_mblk = blk.value, par, mblk.value
        assert self.d_own and self.d_mblk and self.par.value

    def _get(self, ptr, n=16):
        out = np.empty(n)
        self.z.q._copy(out.ctypes.data, ptr, 8 * n, 2)
        return out

    def _put(self, ptr, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        self.z.q._copy(ptr, a.ctypes.data, a.nbytes, 1)

    own = lambda self: self._get(self.d_own)
    mblk = lambda self: self._get(self.d_mblk)
    upload_own = lambda self, a: self._put(self.d_own, a)
    upload_mblk = lambda self, a: self._put(self.d_mblk, a)

    def call(self, name, *args):
        self.S.check(getattr(self.S.L, "iem_rmu_" + name)(self.rp, *args))

    def state(self):
        from infiniteexamodels.jl_amd import lib as iemlib
        v = iemlib.RmuState()
        v.struct_size = C.sizeof(iemlib.RmuState)
        self.S.check(self.S.L.iem_rmu_state(self.rp, C.byref(v)))
        return v

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if self.rp is not None:
            self.S.check(self.S.L.iem_rmu_destroy(self.rp))
            self.rp = None
        return False


@contextlib.contextmanager
def original_mu(S, **opts):
    """a raw iem_mu object on the layer's barrier object: ``(handle, address of its block)``"""
    from infiniteexamodels.jl_amd import lib as iemlib
    o = iemlib.MuOpts.defaults(**opts)
    p, blk = C.c_void_p(), C.c_void_p()
    S.check(S.L.iem_mu_create(S.b, C.byref(o), C.byref(p)))
    try:
        S.check(S.L.iem_mu_device(p, C.byref(blk)))
        yield p, blk.value
    finally:
        S.check(S.L.iem_mu_destroy(p))


def mid_phase(name, S):
    """the shared middle of a phase of tests/test_gpu_resto.py: ``(R, host state, mu, r, c)``"""
    P = S.P
    if name in BIG:
        E = rref.big_entered(BIG[name])
        R, st_h, mu = {k: v.copy() for k, v in E["R"].items()}, E["state"], E["mu"]
        r_h = P["r"]
    else:
        R, st_h, mu = rref.entered(P)
        r_h = P["om"].jtprod(st_h[0], st_h[2])
    blk = R["blk"].copy()
    blk.view(np.int64)[0] = rref.ACTIVE
    blk[rref.R_THETA_START] = 2.0
    R["blk"] = blk
    return R, st_h, mu, r_h, P["c"]


def spots(S, what):
    """``[(label, entry)]``: the nearest entry of kind `what` to entry 0, nvar − 1, the first row, n − 1, both sides of entry 4096·256 and
    the first entry of a third trip, each listed once"""
    B = S.B
    no_x, no_s = np.zeros(S.nvar, dtype=bool), np.zeros(S.ncon, dtype=bool)
    mask = {"variable": np.concatenate([~no_x, no_s]), "row": np.concatenate([no_x, ~no_s]), "inequality row": np.concatenate([no_x, ~B["eq"]]),
            "lower": np.concatenate([B["hasL"], B["gL"]])}[what]
    T = 4096 * 256
    pos = {"0": 0, "nvar - 1": S.nvar - 1, "the first row": S.nvar, "n - 1": S.n - 1}
    if S.n > T:
        pos.update({"2^20 - 1": T - 1, "2^20": T})
    if S.n > 2 * T:
        pos["first of trip three"] = 2 * T
    out, seen = [], set()
    if not mask.any():
        return out
    for label, i in pos.items():
        k = bref.nearest(mask, i)
        if k not in seen:
            seen.add(k)
            out.append((f"{label} -> {k}", k))
    return out


# ---- (a) iem_rmu_error ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS + list(BIG))
def test_error_bitwise(name, built):
    with layer(name) as S, contextlib.ExitStack() as stack:
        B = S.B
        n, m = S.nvar, S.ncon
        if name in BIG:
            big_facts(name, S)
        q = S.search()
        z = S.resto(q)
        rp = stack.enter_context(Rmu(S, z))
        R, st_h, mu, r_h, c_h = mid_phase(name, S)
        z.upload(R)
        st = tuple(dev(a) for a in st_h)
        r, c = dev(r_h), dev(c_h)
        mblk = mref.fresh_block(dict(qref.OPTS, mu_init=mu))
        mblk[3:8] = NAN      # (never read)
        rp.upload_mblk(mblk)
        own0 = rp.own()
        mus, zetas = qref.ladder(mblk)

        def device_words():
            out = nan(32)
            rp.call("error", *map(_p, st), _p(r), _p(c), _p(out))
            return host(out, 32)

        def unbound(mu_k, zeta_k):
            out = nan(8)
            z.call("error", *map(_p, st), _p(r), _p(c), float(mu_k), float(zeta_k), _p(out))
            return host(out, 8)

        def against_the_device(w, what):
            """words 0–7 and every candidate's maxima against UNBOUND iem_resto_error calls on the device"""
            assert same_bits(w[:8], unbound(0.0, zetas[0])), what
            for k in range(qref.K):
                e = unbound(mus[k], zetas[k])
                assert same_bits(w[12 + 3 * k], mus[k]) and same_bits(w[13 + 3 * k:15 + 3 * k], e[:2]), (what, k, w[12 + 3 * k:15 + 3 * k], e[:2])
            assert same_bits(w[11], 0.0) and same_bits(w[30:], [0.0, 0.0]), what

        w = device_words()
        assert same_bits(device_words(), w)      # the same bits every time
        against_the_device(w, "base")
        ref = qref.error_device(B, R, st_h, r_h, c_h, mblk, S.info["workgroups"])
        print(name, "rmu_error:", w.tolist())
        print(name, "reference:", ref.tolist())
        assert same_bits(w[:7], ref[:7]) and same_bits(w[8:], ref[8:]), (w, ref)
        logs_within(float(w[7]), ref[7], rref.error(B, R, st_h, r_h, c_h, 0.0, float(zetas[0]))[4], "L")
        assert w[10] == 0.0 and 0.0 < w[8] < w[3] and same_bits(rp.own(), own0) and same_bits(rp.mblk(), mblk)      # it writes no block
        # ---- planted extremes, one at a time
        base = w

        def put_vec(offset, value):
            a = np.array([value], dtype=np.float64)
            z.q._copy(z.d_vec + 8 * offset, a.ctypes.data, 8, 1)
        for label, i in spots(S, "variable"):      # r: every candidate's variable maximum
            old = float(r[i])
            r[i] = 1e30
            got = device_words()
            against_the_device(got, ("r", label))
            assert (got[13:30:3] > base[13:30:3]).all() and same_bits(got[14:30:3], base[14:30:3]) and same_bits(got[2:12], base[2:12]), ("r", label)
            r[i] = old
        for label, i in spots(S, "row"):      # y: the row maxima (|rho − y − zp| on every row) and sum |y|; c: max |rc|
            j = i - n
            old = float(st[2][j])
            st[2][j] = 1e30
            got = device_words()
            against_the_device(got, ("y", label))
            assert (got[14:30:3] > base[14:30:3]).all() and same_bits(got[13:30:3], base[13:30:3]), ("y", label)
            st[2][j] = old
            old = float(c[j])
            c[j] = -1e30
            got = device_words()
            against_the_device(got, ("c", label))
            assert got[2] > base[2] and same_bits(got[2], abs((rref.infeasibility(B, np.where(np.arange(m) == j, -1e30, c_h), st_h[1])[j] - R["p"][j]) + R["n"][j])), ("c", label)
            c[j] = old
        for label, i in spots(S, "lower"):      # a product below the minimum, above the maximum, and a NaN
            j, vec, gap = (i, st[3], st_h[0][i] - B["xl"][i]) if i < n else (i - n, st[5], st_h[1][i - n] - B["rl"][i - n])
            old = float(vec[j])
            for value, word in ((1e-30, 8), (1e30, 3)):
                vec[j] = value
                got = device_words()
                against_the_device(got, ("z", label, value))
                assert same_bits(got[word], gap * value) and got[10] == 0.0 and (got[8] < base[8] if word == 8 else got[3] > base[3]), ("z", label, value, got[word], gap * value)
            held_min = same_bits(gap * old, base[8])      # (an entry that held the minimum itself takes it along)
            vec[j] = NAN
            got = device_words()
            against_the_device(got, ("NaN", label))
            assert got[10] == 1.0 and np.isnan(got[3]) and np.isnan(got[9]) and (held_min or same_bits(got[8], base[8])), ("NaN", label)
            assert np.isnan(got[13:30:3] if i < n else got[14:30:3]).all(), ("NaN", label)
            vec[j] = -old
            got = device_words()
            against_the_device(got, ("negative", label))
            assert got[10] == 1.0 and (held_min or same_bits(got[8], base[8])) and same_bits(got[3], base[3]) and got[9] <= base[9], ("negative", label)
            vec[j] = old
        for kind, off, src in (("variable", 12 * m, "xR"), ("inequality row", 10 * m - n, "sR")):      # the zeta term decides: the candidates differ, each by its zeta
            for label, i in spots(S, kind):
                put_vec(off + i, float(R[src][i if i < n else i - n]) - 1e40)
                got = device_words()
                against_the_device(got, (src, label))
                words = got[13:30:3] if i < n else got[14:30:3]
                assert (np.diff(words) < 0).all() and (words > (base[13:30:3] if i < n else base[14:30:3])).all(), (src, label, words)
                put_vec(off + i, float(R[src][i if i < n else i - n]))
        # ... and r cancels the zeta term at zeta_0: candidate 0 keeps the rest's maximum, every later candidate carries the planted entry's
        # |(zeta_k − zeta_0)·wx·(x − xR)|, which GROWS with k — the extreme sits in a candidate other than 0
        for label, i in spots(S, "variable"):
            xr = np.float64(st_h[0][i]) - np.float64(1e30)
            old = float(r[i])
            put_vec(12 * m + i, float(xr))
            r[i] = float(-((zetas[0] * R["wx"][i]) * (st_h[0][i] - xr)))
            got = device_words()
            against_the_device(got, ("cancelled at zeta_0", label))
            words = got[13:30:3]
            assert (np.diff(words[1:]) > 0).all() and words[1] > words[0] and words[0] < 1e20 < words[5], ("cancelled at zeta_0", label, words)
            r[i] = old
            put_vec(12 * m + i, float(R["xR"][i]))
        assert same_bits(device_words(), base)


# ---- (b) bound against unbound ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
def test_bound_against_unbound(name, built):
    with layer(name) as S, contextlib.ExitStack() as stack:
        P, B = S.P, S.B
        n, m = S.nvar, S.ncon
        q = S.search()
        z = S.resto(q)
        rp = stack.enter_context(Rmu(S, z))
        orig, d_orig = stack.enter_context(original_mu(S))
        rp_o = stack.enter_context(Rmu(S, z, orig))
        R, st_h, mu, r_h, c_h = mid_phase(name, S)
        tau, zeta = 0.9375, math.sqrt(mu) * 1.25      # (not what a rule would give: whatever the block holds is what the kernels take)
        mu_orig = 0.0123
        blk = np.full(16, NAN)
        blk[:3] = (mu, tau, zeta)
        rng = np.random.default_rng(47)
        sol_h = rng.standard_normal(S.n)
        ct_h = c_h + 1e-3 * rng.standard_normal(m)
        ctl_o = sref.block(alpha=0.0, alpha_max=1.0, phi0=10.0, theta0=2.0, slope=-1.0, theta_min=1e-4, theta_max=1e4, phi_t=10.5, theta_t=2.5, status=sref.FAILED, trials=30, flags=1,
                           count=2)
        filt_o = sref._filter([(50.0, -1000.0), (3.0, 11.0)], q.cap)
        ictl0 = sref.block(status=sref.UNUSABLE, count=1, flags=1, theta_min=1e-4, theta_max=1e4)
        ifilt0 = sref._filter([(1e9, -1e9)], q.cap)

        def run(bound):
            """the whole sequence; returns everything it wrote"""
            S.check(S.L.iem_resto_bind_mu(z.z, bound.rp if bound else None))
            if bound:
                bound.upload_mblk(blk)
            a = GARBAGE if bound else dict(mu=mu, tau=tau, zeta=zeta)
            seen = []

            def keep(*bufs):
                seen.extend(t.cpu().numpy().copy() for t in bufs)
                R_now = z.object()
                seen.extend(R_now[k] for k in rref.ROWS + rref.VARS + ("blk",))
                seen.extend([z.inner.block(), z.inner.filter(), q.block(), q.filter()])
            q.upload(ctl_o, filt_o)
            z.inner.upload(ictl0, ifilt0)
            z.upload(rref.new_object(n, m))
            st = tuple(dev(t) for t in P["state"])
            c, r, sol, ct = dev(c_h), dev(r_h), dev(sol_h), dev(ct_h)
            z.call("enter", *map(_p, st), _p(c), a["mu"])
            keep(*st)
            z.upload(R)
            st = tuple(dev(t) for t in st_h)
            sigma, dcon, rhs = nan(n), nan(m), nan(S.n)
            z.call("terms", *map(_p, st), _p(r), _p(c), a["mu"], a["zeta"], _p(sigma), _p(dcon), _p(rhs))
            keep(sigma, dcon, rhs)
            dirs, alpha = tuple(nan(k) for k in S.dsizes), nan(2)
            z.call("step", *map(_p, st), _p(sol), a["mu"], a["tau"], a["zeta"], *map(_p, dirs), _p(alpha))
            keep(*dirs, alpha)
            m0 = nan(3)
            z.call("merit", 0, _p(st[0]), _p(st[1]), _p(c), a["zeta"], _p(m0))
            keep(m0)
            z.call("begin", _p(st[0]), _p(st[1]), _p(sol), _p(dirs[0]), _p(m0), _p(alpha), a["mu"], a["zeta"])
            keep()
            xt, s_t, m1 = nan(n), nan(m), nan(3)
            z.call("trial", _p(st[0]), _p(st[1]), _p(sol), _p(dirs[0]), _p(xt), _p(s_t))
            z.call("merit", 1, _p(xt), _p(s_t), _p(ct), a["zeta"], _p(m1))
            keep(xt, s_t, m1)
            out = nan(8)
            z.call("error", *map(_p, st), _p(r), _p(c), a["mu"], a["zeta"], _p(out))
            keep(out)
            z.call("update", *map(_p, st), _p(sol), *map(_p, dirs), _p(alpha), a["mu"], KAPPA)
            keep(*st)
            f, m2 = dev([9.0]), dev([1.0, 0.7])
            # check: with a par_orig the ORIGINAL block's mu rules and the host's is ignored; without one the host's argument stays
            z.call("check", _p(f), _p(m2), a["mu"] if bound is rp_o else mu_orig)
            keep()
            return seen, alpha.cpu().numpy()[:2]

        z.q._copy(d_orig, np.concatenate([[mu_orig], np.full(15, NAN)]).ctypes.data, 128, 1)
        plain, alpha_h = run(None)
        assert 0.0 < alpha_h[0] <= 1.0 and 0.0 < alpha_h[1] <= 1.0
        blk_after = plain[-5]
        assert same_bits(blk_after[rref.R_PHI], 9.0 - mu_orig * 0.7) and blk_after[rref.R_THETA] == 1.0      # the check ran, with the original problem's mu
        for bound, what in ((rp, "bound"), (rp_o, "bound, with a par_orig")):
            got, _ = run(bound)
            assert len(got) == len(plain)
            bad = [k for k, (a, b) in enumerate(zip(got, plain)) if not same_bits(a, b)]
            assert not bad, (what, bad)
            assert same_bits(bound.mblk(), blk)      # no iem_resto_* kernel writes the block
        # unbound again: the host arguments and their range checks are back
        S.check(S.L.iem_resto_bind_mu(z.z, None))
        again, _ = run(None)
        assert all(same_bits(a, b) for a, b in zip(again, plain))
        st = tuple(dev(t) for t in st_h)
        assert S.L.iem_resto_error(z.z, *map(_p, st), None, _p(dev(c_h)), -1.0, 0.3, _p(nan(8))) == -4 and "mu" in S.L.iem_last_error().decode()


# ---- (c) the one-workgroup kernels ------------------------------------------------------------------------------------------------------
def ulps(a, b):
    a, b = np.float64(a), np.float64(b)
    if np.isnan(a) or np.isnan(b):
        return 0 if np.isnan(a) and np.isnan(b) else 2 ** 62
    return abs(int(a.view(np.int64)) - int(b.view(np.int64)))


def test_enter_update_trigger_every_branch(built):
    from test_rmu import trigger_cases, words
    with layer("wb_ineq") as S, contextlib.ExitStack() as stack:
        q = S.search()
        z = S.resto(q)
        rp = stack.enter_context(Rmu(S, z))
        orig, d_orig = stack.enter_context(original_mu(S))
        rp_o = stack.enter_context(Rmu(S, z, orig))
        second, d_second = stack.enter_context(original_mu(S, kappa_eps=10.0, kappa_mu=0.2, tau_min=0.99, tol=1e-8, mu_floor=1e-11, s_max=100.0))
        counts = (S.ncon, S.B["counts"]["nz"] + 2 * S.ncon)
        put = lambda ptr, a: z.q._copy(ptr, np.ascontiguousarray(a, dtype=np.float64).ctypes.data, 8 * len(a), 1)
        empty = sref._filter([(3.0, 4.0)], q.cap)
        # ---- enter
        own0 = np.arange(16, dtype=np.float64) + 1.0
        mblk0 = mref.fresh_block(dict(qref.OPTS, mu_init=0.3))
        mblk0[3:8] = [1.0, 2.0, 3.0, 4.0, 5.0]
        mref.ints(mblk0)[8:12] = [2, 1, 7, 9]
        ictl0 = sref.block(status=sref.F_TYPE, count=7, flags=3, alpha=0.25, theta_min=1e-4)
        err = lambda inf: np.array([9.0, 9.0, inf, 9.0, 9.0, 9.0, 9.0, 9.0])
        oblk = mref.fresh_block(dict(qref.OPTS, mu_init=0.02))
        for label, e, mu_host, ob in (("the infeasibility decides", err(2.5), 0.1, None), ("mu decides", err(0.01), 0.1, None), ("the original block's mu", err(0.01), 0.1, oblk),
                                      ("the original block, the infeasibility decides", err(0.5), 7.0, oblk), ("a NaN infeasibility", err(NAN), 0.1, None), ("a NaN mu", err(0.5), NAN, None),
                                      ("not positive", err(0.0), 0.0, None), ("negative", err(-1.0), -2.0, None), ("a NaN in the original block", err(0.5), 0.1, np.full(16, NAN))):
            obj = rp_o if ob is not None else rp
            if ob is not None:
                put(d_orig, ob)
            obj.upload_own(own0)
            obj.upload_mblk(mblk0)
            z.inner.upload(ictl0, empty)
            obj.call("enter", _p(dev(e)), mu_host)
            want = qref.enter(own0, mblk0, ictl0, e, mu_host, ob)
            got = (obj.own(), obj.mblk(), z.inner.block())
            assert all(same_bits(a, b) for a, b in zip(got, want)), (label, got, want)
            assert same_bits(z.inner.filter(), empty)
        # the restoration block is bitwise iem_mu_reset on a second object
        for mu_r in (2.5, 0.1, 1e-9):
            put(d_second, mblk0)
            S.check(S.L.iem_mu_reset(second, mu_r))
            rp.upload_own(own0)
            rp.upload_mblk(mblk0)
            rp.call("enter", _p(dev(err(mu_r))), 1e-12)
            blk2 = np.empty(16)
            z.q._copy(blk2.ctypes.data, d_second, 128, 2)
            assert same_bits(rp.mblk(), blk2) and blk2[0] == mu_r, mu_r
        # ---- update: every branch of tests/test_rmu.py, on the device
        mu6, _ = qref.ladder(mref.fresh_block(dict(qref.OPTS, mu_init=0.1)))
        cases = [("unusable by count", words(bad=1.0)), ("unusable by NaN", words(d=(NAN,) * 6)), ("a NaN infeasibility", words(inf=NAN)), ("stationary", words(mu0=1e-9, d=(1e-9,) * 6)),
                 ("no decrease", words(mu0=0.1, d=(2.0,) * 6)), ("a NaN candidate", words(mu0=0.1, d=(1e-4, 1e-4, NAN, 1e-4, 1e-4, 1e-4), pmax=0.0, pmin=0.0))]
        for stop in (1, 2, 3, 4, 5, 6):      # (6: truncated)
            d = tuple((5.0 if k < stop else 20.0) * mu6[k] for k in range(6))
            cases.append((f"{min(stop, 5)} decreases" + (", truncated" if stop == 6 else ""), words(mu0=0.1, d=d, pmax=0.0, pmin=0.0)))
        cases.append(("at the floor", words(mu0=1e-11, d=(1e-4,) * 6, pmax=0.0, pmin=0.0)))
        own_run = qref.fresh_own()
        seen = set()
        for label, (w, blk) in cases:
            ictl = sref.block(status=sref.F_TYPE, count=7, flags=3, alpha=0.25)
            rp.upload_own(own_run)
            rp.upload_mblk(blk)
            z.inner.upload(ictl, empty)
            rp.call("update", _p(dev(w)))
            want = qref.update(own_run, blk, ictl, w, counts)
            got = (rp.own(), rp.mblk(), z.inner.block())
            assert all(same_bits(a, b) for a, b in zip(got, want)), (label, got, want)
            moved = bool(qref.ints(got[0])[qref.FLAGS] & 1)
            assert moved == (not same_bits(got[1], blk)) == (sref.word(got[2], sref.COUNT) == 0), label      # the filter goes exactly when mu moved
            seen.add((int(qref.ints(got[0])[qref.STATUS]), int(qref.ints(got[0])[qref.FLAGS]), int(qref.ints(got[0])[qref.LAST])))
            own_run = got[0]      # (the total runs on)
            st = rp.state()
            assert (st.status, st.flags, st.decreases_last, st.decreases) == tuple(int(v) for v in qref.ints(got[0])[:4]) and same_bits([st.e0, st.e_mu, st.mu, st.tau, st.zeta],
                                                                                                                                        [got[0][4], got[0][5], got[1][0], got[1][1], got[1][2]]), label
        assert seen >= {(2, 0, 0), (1, 0, 0), (0, 0, 0), (0, 1, 1), (0, 1, 2), (0, 1, 3), (0, 1, 4), (0, 1, 5), (0, 3, 5)}, seen
        assert qref.ints(own_run)[qref.TOTAL] == 1 + 2 + 3 + 4 + 5 + 5 + 2
        # ---- trigger: every case of tests/test_rmu.py on both searches
        for which, search in ((0, q), (1, z.inner)):
            own0 = qref.fresh_own()
            own0[qref.ALPHA_MIN] = 77.0
            qref.ints(own0)[qref.TRIG_ORIG], qref.ints(own0)[qref.TRIG_INNER] = 4, 9
            for label, ctl, fires in trigger_cases():
                rp.upload_own(own0)
                search.upload(ctl, empty)
                alpha = dev([0.625, 0.5])
                rp.call("trigger", which, _p(alpha))
                own_w, ctl_w, a0 = qref.trigger(own0, ctl, which)
                own_g, ctl_g, alpha_g = rp.own(), search.block(), host(alpha, 2)
                d = ulps(own_g[qref.ALPHA_MIN], own_w[qref.ALPHA_MIN])
                print(f"  trigger {which} {label}: alpha_min {own_g[qref.ALPHA_MIN]!r} against {own_w[qref.ALPHA_MIN]!r} ({d} ulp), fires {fires}")
                assert d <= 4, (label, d)
                own_g[qref.ALPHA_MIN] = own_w[qref.ALPHA_MIN]
                assert same_bits(own_g, own_w) and same_bits(ctl_g, ctl_w) and same_bits(alpha_g, [0.625 if a0 is None else a0, 0.5]) and same_bits(search.filter(), empty), label
                rp.call("trigger", which, _p(alpha))      # idempotent
                own_2 = rp.own()
                assert ulps(own_2[qref.ALPHA_MIN], own_w[qref.ALPHA_MIN]) <= 4
                own_2[qref.ALPHA_MIN] = own_w[qref.ALPHA_MIN]
                assert same_bits(own_2, own_w) and same_bits(search.block(), ctl_w) and same_bits(host(alpha, 2), alpha_g), label
        # ---- state: one copy brings the three blocks home
        rb = np.zeros(8)
        rb.view(np.int64)[0] = rref.ACTIVE
        rb[1:4] = (2.0, 1.5, -7.0)
        put(z.d_blk, rb)
        st = rp.state()
        own, mb = rp.own(), rp.mblk()
        assert (st.resto_state, st.theta_start, st.theta, st.phi) == (rref.ACTIVE, 2.0, 1.5, -7.0) and (st.triggers_orig, st.triggers_inner) == tuple(int(v) for v in qref.ints(own)[9:11])
        assert same_bits([st.mu, st.tau, st.zeta, st.mu_e0, st.mu_e_mu, st.mu_e_d, st.mu_e_p, st.mu_e_c0], mb[:8]) and same_bits(st.alpha_min, own[8])
        assert (st.mu_status, st.mu_flags, st.mu_decreases, st.mu_updates) == tuple(int(v) for v in mref.ints(mb)[8:12])


# ---- (f) the refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals(built):
    from infiniteexamodels.jl_amd import lib as iemlib
    with layer("wb_ineq") as S, layer("wb_eq") as S2, contextlib.ExitStack() as stack:
        L = S.L
        err = lambda: L.iem_last_error().decode()
        q, q2 = S.search(), S2.search()
        z, z_other, z2 = S.resto(q), S.resto(q), S2.resto(q2)
        out = C.c_void_p()
        for name in qref.OPTS:
            for v in [0.0, -1.0, NAN, float("inf")] + ([1.0] if name in ("kappa_mu", "tau_min", "gamma_alpha") else []):
                o = iemlib.RmuOpts.defaults(**{name: v})
                assert L.iem_rmu_create(z.z, None, C.byref(o), C.byref(out)) == -4 and name in err() and not out.value, (name, v)
        o = iemlib.RmuOpts.defaults()
        o.struct_size = 4
        assert L.iem_rmu_create(z.z, None, C.byref(o), C.byref(out)) == -4 and "struct_size" in err()
        assert L.iem_rmu_create(z.z, None, None, None) == -4 and "null" in err()
        foreign, _ = stack.enter_context(original_mu(S2))
        assert L.iem_rmu_create(z.z, foreign, None, C.byref(out)) == -4 and "another barrier object" in err() and not out.value
        rp = stack.enter_context(Rmu(S, z))      # NULL options: the defaults
        assert L.iem_resto_bind_mu(z_other.z, rp.rp) == -4 and "another iem_resto" in err()
        assert L.iem_resto_bind_mu(z2.z, rp.rp) == -4 and "another iem_resto" in err()
        st = tuple(dev(a) for a in S.P["state"])
        p = list(map(_p, st))
        c, r, o32, a2 = dev(S.P["c"]), dev(S.P["r"]), nan(32), nan(2)
        assert L.iem_rmu_error(rp.rp, *p, None, _p(c), _p(o32)) == -4 and "null" in err()      # r is required
        assert L.iem_rmu_error(rp.rp, *p, _p(r), None, _p(o32)) == -4 and "null" in err()
        assert L.iem_rmu_error(rp.rp, *p, _p(r), _p(c), None) == -4 and "null" in err()
        assert L.iem_rmu_error(rp.rp, p[0], None, *p[2:], _p(r), _p(c), _p(o32)) == -4 and "null" in err()      # s with inequality rows
        assert L.iem_rmu_enter(rp.rp, None, 0.1) == -4 and "null" in err()
        assert L.iem_rmu_update(rp.rp, None) == -4 and "null" in err()
        assert L.iem_rmu_trigger(rp.rp, 0, None) == -4 and "null" in err()
        assert L.iem_rmu_trigger(rp.rp, 2, _p(a2)) == -4 and "which" in err()
        assert np.isnan(host(o32, 32)).all() and np.isnan(host(a2, 2)).all()      # refused before any device work
        v = iemlib.RmuState()
        v.struct_size = 4
        assert L.iem_rmu_state(rp.rp, C.byref(v)) == -4 and "struct_size" in err()
        # a shorter struct: at most that many bytes are written
        v = iemlib.RmuState()
        v.struct_size = 5 * 8
        v.e0 = 123.0
        assert L.iem_rmu_state(rp.rp, C.byref(v)) == 0 and v.e0 == 123.0 and v.status == 0
        # destroy unbinds: the unbound calls and their range checks are back
        S.check(L.iem_resto_bind_mu(z.z, rp.rp))
        S.check(L.iem_search_bind_mu(z.inner.s, rp.par))
        rp.__exit__()
        assert L.iem_resto_error(z.z, *p, _p(r), _p(c), -1.0, 0.3, _p(nan(8))) == -4 and "mu" in err()
        o8 = nan(8)
        S.check(L.iem_resto_error(z.z, *p, _p(r), _p(c), 0.1, 0.3, _p(o8)))
        assert not np.isnan(host(o8, 8)).any()


# ---- (d) one graph ------------------------------------------------------------------------------------------------------------------------
def test_one_bound_iteration_in_one_graph(built):
    """eval_residual(0); rmu_error; rmu_update; jac_hess_coord(0); resto_terms; assemble; iem_kkt_factor_async; refined solve; resto_step;
    merit(0); begin; 6 × {trial, cons, merit(1), accept, rmu_trigger}; update; obj; cons; barrier_merit; check — on wb_eq, entered at the
    shared state, BOUND, captured ONCE and replayed at two states whose updates differ (no decrease; two decreases), loaded by
    device-to-device copies: each replay is bitwise the eager UNBOUND sequence with the values rmu_reference.update gives on the host"""
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.barrier import BarrierLayer, FilterSearch, Restoration, RestorationParameter
    from infiniteexamodels.jl_amd.kkt_chain import KKTObject
    from infiniteexamodels.jl_amd.model import ExaModel
    P = rref.point("wb_eq")
    B = P["B"]
    gm = ExaModel(P["core"], device=0, blob=P["blob"])
    n, m = P["om"].nvar, P["om"].ncon
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    new = lambda k: torch.full((k,), NAN, dtype=torch.float64, device="cuda")
    zeros = lambda k: torch.zeros(k, dtype=torch.float64, device="cuda")
    S_check = iemlib.check

    def d2d(dst, src, k):
        assert hip().hipMemcpy(dst, src, 8 * k, 3) == 0
    try:
        with BarrierLayer(gm) as bar, KKTObject(gm) as kkt, FilterSearch(bar) as fs, Restoration(fs) as resto, RestorationParameter(resto) as rp:
            counts_r = (bar.info["ncon"], bar.info["nz"] + 2 * bar.info["ncon"])
            state = tuple(T(np.where(np.isnan(a), 0.0, a)) for a in P["state"])
            x, s, y = state[0], state[1], state[2]
            c, r, f = new(m), new(n), new(1)
            jv, hv = new(int(gm.meta.nnzj)), new(int(gm.meta.nnzh))
            sigma, dcon, rhs, sol = new(n), new(m), new(n + m), new(n + m)
            dirs, alpha = (zeros(m), new(n), new(n), zeros(m), zeros(m)), new(2)
            xt, st, ct, m3, mt3, m2, w32 = new(n), zeros(m), new(m), new(3), new(3), new(2), new(32)
            inertia = torch.zeros(3, dtype=torch.int64, device="cuda")
            outputs = (c, r, f, sigma, dcon, rhs, sol, alpha, xt, ct, m3, mt3, m2, w32, dirs[1], dirs[2])
            gm.cons(x, c)
            with np.errstate(invalid="ignore"):
                mu_e = max(0.1, float(np.abs(rref.infeasibility(B, P["om"].cons(P["state"][0]), P["state"][1])).max()))
            resto.enter(state, c, mu_e)
            resto.inner.reset()
            torch.cuda.synchronize()
            ptr = resto.device()
            ictl, iflt = resto.inner.device()
            cap = int(fs.opts["filter_capacity"])
            nvec = 12 * m + 2 * n
            places = [(ptr["p"], nvec), (ptr["block"], 8), (ictl, 16), (iflt, 2 * cap), (rp.device(), 16), (rp.inner_mu.device(), 16)]
            L, k = kkt._handle()

            def snapshot():
                torch.cuda.synchronize()
                saved = [t.clone() for t in state]
                for p_, k_ in places:
                    t = torch.empty(k_, dtype=torch.float64, device="cuda")
                    d2d(t.data_ptr(), p_, k_)
                    saved.append(t)
                torch.cuda.synchronize()
                return saved

            def load(saved):
                torch.cuda.synchronize()
                for t, a in zip(state, saved[:7]):
                    t.copy_(a)
                for (p_, k_), a in zip(places, saved[7:]):
                    d2d(p_, a.data_ptr(), k_)
                for t in outputs:
                    t.fill_(NAN)
                torch.cuda.synchronize()

            def at_mu(mu0):
                """the entered state with the restoration block reset to mu0 and the own block zero"""
                load(start)
                rp.inner_mu.reset(mu0)
                torch.cuda.synchronize()
                assert hip().hipMemcpy(rp.device(), np.zeros(16).ctypes.data, 128, 1) == 0
                return snapshot()

            def iteration(a):
                """a = None: bound; otherwise the host's (mu, tau, zeta) for the unbound calls"""
                mu_, tau_, zeta_ = a if a else (GARBAGE["mu"], GARBAGE["tau"], GARBAGE["zeta"])
                gm.eval_residual(x, y, 0.0, c=c, out=r, obj=f)
                rp.error(state, r, c, out=w32)
                rp.update(w32)
                gm.jac_hess_coord(x, y, jv, hv, obj_weight=0.0)
                resto.terms(state, r, c, mu_, zeta_, out=(sigma, dcon, rhs))
                kkt.assemble(hv, jv, sigma, 0.0, DELTA_C, dcon=dcon, at=(x, y, 0.0))
                S_check(L.iem_kkt_factor_async(k, _p(inertia)))
                S_check(L.iem_kkt_solve_refined_diag(k, _p(x), _p(y), 0.0, _p(sigma), _p(dcon), 0.0, DELTA_C, 1, _p(rhs), n + m, _p(sol), n + m, 1, None))
                resto.step(state, sol, mu_, tau_, zeta_, out=dirs, alpha=alpha)
                resto.merit(0, x, s, c, zeta_, out=m3)
                resto.begin(state, sol, dirs[0], m3, alpha, mu_, zeta_)
                for _ in range(6):
                    resto.trial(state, sol, dirs[0], xt, st)
                    gm.cons(xt, ct)
                    resto.merit(1, xt, st, ct, zeta_, out=mt3)
                    resto.inner.accept(mt3[0:1], mt3[1:3], mu_ if a else 0.0, alpha)
                    rp.trigger(1, alpha)
                resto.update(state, sol, dirs, alpha, mu_)
                gm.obj_device(x, out=f)
                gm.cons(x, c)
                bar.merit(x, s, c, out=m2)
                resto.check(f, m2, 0.1)

            def results():
                torch.cuda.synchronize()
                return [t.clone() for t in state + outputs + dirs] + snapshot()[7:] + [inertia.clone().double()]

            start = snapshot()
            # two states whose updates differ: scan mu0, the restated rule deciding on the words the device forms
            found = {}
            for e in range(24, -33, -1):
                mu0 = 10.0 ** (e / 8.0)
                saved = at_mu(mu0)
                gm.eval_residual(x, y, 0.0, c=c, out=r, obj=f)
                rp.error(state, r, c, out=w32)
                torch.cuda.synchronize()
                own, mblk, _ = qref.update(qref.fresh_own(), saved[-1].cpu().numpy(), sref.block(), w32.cpu().numpy(), counts_r)
                j = int(qref.ints(own)[qref.LAST])
                if qref.ints(own)[qref.STATUS] == qref.ITERATING and j in (0, 2) and j not in found:
                    found[j] = (mu0, saved, tuple(float(v) for v in mblk[:3]))
            print("wb_eq: mu0 with no decrease", found.get(0, (None,))[0], "with two decreases", found.get(2, (None,))[0])
            assert set(found) == {0, 2}, found.keys()
            # eager, unbound, with the host's values
            eager = {}
            for j, (mu0, saved, host_values) in found.items():
                load(saved)
                iteration(host_values)
                eager[j] = results()
                own_after, mblk_after = eager[j][-3].cpu().numpy(), eager[j][-2].cpu().numpy()
                assert int(qref.ints(own_after)[qref.LAST]) == j and same_bits(mblk_after[:3], host_values) and (j == 0) == (mblk_after[0] == mu0)
                status = sref.word(eager[j][-5].cpu().numpy(), sref.STATUS)
                print(f"  {j} decreases: mu {mu0!r} -> {mblk_after[0]!r}, inertia {eager[j][-1].tolist()}, inner status {status}, alpha {eager[j][14].tolist()}")
                assert eager[j][-1].tolist()[1:] == [m, 0] and not torch.equal(eager[j][0], saved[0])      # the iterate moved
            assert not torch.equal(eager[0][0], eager[2][0])      # ... and differently at the two states
            # bound, captured once
            resto.bind_mu(rp)
            resto.inner.bind_mu(rp.inner_mu)
            load(found[0][1])
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                gm._sync_stream()
                iteration(None)
            gm._sync_stream()
            for j in (0, 2, 2, 0):
                load(found[j][1])
                graph.replay()
                again = results()
                bad = [i for i, (a, b) in enumerate(zip(again, eager[j])) if not torch.equal(a.view(torch.int64), b.view(torch.int64))]
                assert not bad, (j, bad)
            # bound and eager: the same bits once more
            load(found[2][1])
            iteration(None)
            again = results()
            assert all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip(again, eager[2]))
            resto.inner.bind_mu(None)
            resto.bind_mu(None)
    finally:
        gm.close()


# ---- (e) the loop -----------------------------------------------------------------------------------------------------------------------
def _loop_model(name):
    from infiniteexamodels.jl_amd import transcribe
    if name == "classical":
        return transcribe.exa_core(rref.wachter_biegler(-1.0, 0.5, 3, False, start=(-2.0, 3.0, 1.0)))
    return rref.wb_core(name)


@pytest.mark.parametrize("name", list(rref.WB_MODELS) + ["classical"])
def test_the_loop_on_the_device_and_on_the_host(name, built):
    """tests/rmu_loop.py: the rule, the STATIONARY exit and the trigger on the device against the same words read back and
    rmu_reference deciding on the host — bitwise the same iterates; optima 1 and 2 to the tolerances of tests/test_gpu_resto.py; the
    classical model ends STATIONARY both ways.  Iteration and accept counts are printed beside the host reference loop's."""
    import rmu_loop
    from infiniteexamodels.jl_amd.model import ExaModel
    from pyoracle import OracleModel
    core = _loop_model(name)
    blob = core.to_blob()
    gm = ExaModel(core, device=0, blob=blob)
    try:
        dev_ = rmu_loop.solve(gm, decide="device")
        hst = rmu_loop.solve(gm, decide="host")
    finally:
        gm.close()
    ref = qref.host_loop(OracleModel(blob))
    show = lambda o: {k: o[k] for k in ("status", "iterations", "error", "objective", "restorations", "resto_iterations", "why", "accepts", "triggers", "decreases", "truncated")}
    print(name, "device:   ", show(dev_))
    print(name, "host:     ", show(hst))
    print(name, "reference:", show(ref))
    assert len(dev_["iterates"]) == len(hst["iterates"]) and all(same_bits(a, b) for a, b in zip(dev_["iterates"], hst["iterates"]))
    for k in ("status", "iterations", "restorations", "resto_iterations", "why", "decreases", "truncated", "triggers", "accepts"):
        assert dev_[k] == hst[k], k
    assert same_bits(dev_["x"], hst["x"]) and same_bits(dev_["e0"], hst["e0"]) and not dev_["truncated"]
    if name == "classical":
        assert dev_["status"] == "locally infeasible" and dev_["why"] == "stationary" and dev_["error"] > 1e-8 and dev_["e0"][-1] <= 1e-8
        assert ref["status"] == "locally infeasible"
    else:
        optimum = rref.WB_MODELS[name]["optimum"]
        assert dev_["status"] == "solved" and dev_["restorations"] >= 1 and dev_["error"] <= 1e-8 and abs(dev_["objective"] / optimum - 1.0) <= 1e-6
        assert ref["status"] == "solved"
