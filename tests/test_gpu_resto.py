"""The feasibility restoration phase (iem_resto_*, csrc/iem_resto_device.h) on the MI355X.

BITWISE against tests/resto_reference.py (the numpy restatement, no tolerance): every output vector of every kernel — the object's
own vectors read back through hipMemcpy — the step lengths, the maxima, the blocks and the filters; entries that must NOT be written
(the slack side on equality rows, everything under +0.0 step lengths or a FAILED / UNUSABLE inner search, the object under a check
that does not apply) are NaN-poisoned on the way in and compared bit for bit.  THE PARKED SUMS are bitwise too: resto_merit's
rho·S0 + zeta/2·S1 and theta_R, the slope of resto_begin — so the WHOLE inner block, from the restatement's own slope — and sum |y|
and the sum of the multipliers of resto_error carry the bits of resto_reference.merit_device / slope / error_sums, the restatement
in the DEVICE'S ORDER (barrier_reference.device_sum) on the object's own grid of info["workgroups"] workgroups.  ONE EXCEPTION: L, the
sum of logs — the device's log and numpy's need not agree in the last bit, so that column is formed in the device's order from
numpy's logs and compared within barrier_reference.sum_bound, as against math.fsum before; resto_error's copy still carries the bits
of resto_merit(0)'s.  resto_enter's sqrt is compared bitwise as well: the device's f64 sqrt is correctly rounded, as numpy's is.

Models: opf_7, pandemic_20x3, quadrotor_100 (several workgroups, the nvar seam inside one), pandemic_100x7 (47 workgroups: one full
ticket group of iem_last_arrival and one ragged one) of tests/cases.py and the two Waechter-Biegler models of
tests/resto_reference.py at three supports; and THE BIG SHAPES of tests/test_gpu_barrier.py — quadrotor(27 000) and quadrotor(60 000)
of barrier_reference.big_point at resto_reference.big_entered, 4096 workgroups, two and three trips of the stride loop (asserted and
printed) — through every 256-thread kernel, with each extreme slot (resto_step's step lengths, resto_error's maxima, resto_leave_max)
planted at the seam positions of the later trips.  The tables of return-test and filter-append cases are those of
tests/test_resto.py.  One restoration iteration is captured as ONE graph and replayed; tests/resto_loop.py reaches the optima of
the two Waechter-Biegler models, and ends FAILED with max_restorations = 0."""
import contextlib
import ctypes as C
import math
import types

import numpy as np
import pytest

import barrier_reference as bref
import resto_reference as rref
import search_reference as sref
from barrier_reference import KAPPA, TAU
from test_gpu_barrier import BIG, big_facts
from test_gpu_search import NAN, Search, _p, dev, hip, host, nan, same_bits

pytestmark = pytest.mark.gpu
MODELS = ["opf_7", "pandemic_20x3", "quadrotor_100", "pandemic_100x7", "wb_eq", "wb_ineq"]
DELTA_C = 1e-10


class Resto:
    """the raw restoration object of a search: create / destroy, its vectors and block read and written through hipMemcpy, and the
    inner search as a tests/test_gpu_search.py Search"""

    def __init__(self, S, q, **opts):
        from infiniteexamodels.jl_amd import lib as iemlib
        self.S, self.q, self.opts = S, q, dict(rref.OPTS, **opts)
        o = iemlib.RestoOpts.defaults(**opts)
        self.z = C.c_void_p()
        S.check(S.L.iem_resto_create(q.s, C.byref(o), C.byref(self.z)))
        ptr = [C.c_void_p() for _ in range(5)]
        S.check(S.L.iem_resto_device(self.z, *[C.byref(a) for a in ptr]))
        self.d_vec, self.d_blk = ptr[0].value, ptr[4].value
        m = S.ncon
        assert [a.value for a in ptr[:4]] == [self.d_vec + 8 * k * m for k in range(4)] and self.d_blk
        inner = C.c_void_p()
        S.check(S.L.iem_resto_search(self.z, C.byref(inner)))
        self.inner = Search.__new__(Search)
        self.inner.S, self.inner.opts, self.inner.s = S, q.opts, inner
        ctl, flt = C.c_void_p(), C.c_void_p()
        S.check(S.L.iem_search_device(inner, C.byref(ctl), C.byref(flt)))
        self.inner.ctl, self.inner.flt, self.inner.cap = ctl.value, flt.value, q.cap
        assert self.inner.ctl not in (None, q.ctl) and self.inner.flt not in (None, q.flt)

    def object(self):
        """the object as the dict of tests/resto_reference.py"""
        n, m = self.S.nvar, self.S.ncon
        flat = np.empty(12 * m + 2 * n)
        self.q._copy(flat.ctypes.data, self.d_vec, flat.nbytes, 2)
        R = {k: flat[i * m:(i + 1) * m].copy() for i, k in enumerate(rref.ROWS)}
        R.update({k: flat[12 * m + i * n:12 * m + (i + 1) * n].copy() for i, k in enumerate(rref.VARS)})
        R["blk"] = np.empty(8)
        self.q._copy(R["blk"].ctypes.data, self.d_blk, 64, 2)
        return R

    def upload(self, R):
        flat = np.ascontiguousarray(np.concatenate([R[k] for k in rref.ROWS + rref.VARS]), dtype=np.float64)
        assert flat.shape == (12 * self.S.ncon + 2 * self.S.nvar,)
        self.q._copy(self.d_vec, flat.ctypes.data, flat.nbytes, 1)
        blk = np.ascontiguousarray(R["blk"], dtype=np.float64)
        self.q._copy(self.d_blk, blk.ctypes.data, 64, 1)

    def call(self, name, *args):
        self.S.check(getattr(self.S.L, "iem_resto_" + name)(self.z, *args))

    def close(self):
        if self.z is not None:
            self.S.check(self.S.L.iem_resto_destroy(self.z))
            self.z = None


@contextlib.contextmanager
def layer(name, seed=0):
    """tests/test_gpu_search.py's layer with the Waechter-Biegler models among the models"""
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.model import ExaModel
    P = bref.big_point(BIG[name]) if name in BIG else rref.point(name, seed)
    gm = ExaModel(P["core"], device=0, blob=P["blob"]) if P["blob"] is not None else ExaModel(P["core"], device=0)
    b = C.c_void_p()
    bounds = [np.ascontiguousarray(P[k], dtype=np.float64) for k in ("lvar", "uvar", "lcon", "ucon")] if name in BIG else [None] * 4
    iemlib.check(gm._L.iem_barrier_create(gm._h, *[a.ctypes.data if a is not None else None for a in bounds], bref.RELAX, C.byref(b)))
    made = []
    try:
        info = iemlib.BarrierInfo()
        info.struct_size = C.sizeof(iemlib.BarrierInfo)
        iemlib.check(gm._L.iem_barrier_info(b, C.byref(info)))
        cn = P["B"]["counts"]
        S = types.SimpleNamespace(gm=gm, L=gm._L, b=b, P=P, B=P["B"], nvar=cn["nvar"], ncon=cn["ncon"], n=cn["nvar"] + cn["ncon"], check=iemlib.check,
                                  info={k: int(getattr(info, k)) for k, _ in iemlib.BarrierInfo._fields_})
        assert S.nvar == int(gm.meta.nvar) and S.ncon == int(gm.meta.ncon) and S.info["workgroups"] == min(-(-S.n // 256), 4096)
        S.sizes = (S.nvar, S.ncon, S.ncon, S.nvar, S.nvar, S.ncon, S.ncon)
        S.dsizes = (S.ncon, S.nvar, S.nvar, S.ncon, S.ncon)
        S.search = lambda **opts: made.append(Search(S, **opts)) or made[-1]
        S.resto = lambda q, **opts: made.append(Resto(S, q, **opts)) or made[-1]
        gm._sync_stream()
        yield S
    finally:
        for q in reversed(made):      # a restoration object before the search it borrows
            q.close()
        iemlib.check(gm._L.iem_barrier_destroy(b))
        gm.close()


def same_object(got, want, keys=rref.ROWS + rref.VARS + ("blk",)):
    bad = [k for k in keys if not same_bits(got[k], want[k])]
    assert not bad, bad
    return True


def logs_within(got, want, terms, what):
    """a sum of logs: within sum_bound of the device's order over numpy's logs, and of math.fsum"""
    fs, bound = bref.sum_bound(terms)
    print(f"    {what}: device {got!r}, device order over numpy's logs {float(want)!r}, fsum {fs!r}, bound {bound:.3e}, terms {len(terms)}")
    assert abs(got - float(want)) <= bound and abs(got - fs) <= bound, what


def check_merit(S, R, which, x_h, s_h, c_h, zeta, got, what):
    """resto_merit: out[0], out[1] carry the bits of the restatement in the device's order; out[2] is a sum of logs"""
    want = rref.merit_device(S.B, R, which, x_h, s_h, c_h, zeta, S.info["workgroups"])
    print(f"  {what}: device {got.tolist()}, device order {want.tolist()}, workgroups {S.info['workgroups']}")
    assert same_bits(got[:2], want[:2]), (what, got, want)
    logs_within(float(got[2]), want[2], rref.merit_terms(S.B, R, which, x_h, s_h, c_h)[3], "L")


@pytest.mark.parametrize("name", MODELS + list(BIG))
def test_every_kernel_bitwise(name, built):
    with layer(name) as S:
        P, B = S.P, S.B
        n, m = S.nvar, S.ncon
        if name in BIG:
            big_facts(name, S)
        if name == "pandemic_100x7":
            assert S.n == 12000 and S.info["workgroups"] == 47
        eqnan = lambda a: np.where(B["eq"], NAN, a)
        rng = np.random.default_rng(41)
        q = S.search()
        z = S.resto(q)
        R0 = z.object()
        assert same_object(R0, rref.new_object(n, m))      # create zeroes everything; state NONE
        # ---- enter: from the shared state, with the ORIGINAL block of a failed search and two filter entries
        c_h = P["c"]
        with np.errstate(invalid="ignore"):
            mu_e = max(P["mu"], float(np.abs(rref.infeasibility(B, c_h, P["state"][1])).max()))
        ctl_o = sref.block(alpha=0.0, alpha_max=1.0, phi0=10.0, theta0=2.0, slope=-1.0, theta_min=1e-4, theta_max=1e4, phi_t=10.5, theta_t=2.5, status=sref.FAILED, trials=30,
                           flags=1, count=2)
        filt_o = sref._filter([(50.0, -1000.0), (3.0, 11.0)], q.cap)
        q.upload(ctl_o, filt_o)
        st = tuple(dev(a) for a in P["state"])
        c = dev(c_h)
        z.call("enter", *map(_p, st), _p(c), mu_e)
        R1, st1 = rref.enter(B, R0, P["state"], c_h, mu_e)
        R1["blk"], ctl1, filt1 = rref.enter_filter(R0["blk"], ctl_o, filt_o, q.opts)
        got = z.object()
        assert same_object(got, R1)
        assert not got["sR"][B["eq"]].any() and not got["ws"][B["eq"]].any() and not any(got[k].any() for k in ("dp", "dn", "dzp", "dzn", "pt", "nt"))
        for t, want, k in zip(st, st1, S.sizes):
            assert same_bits(host(t, k), want)
        assert same_bits(q.block(), ctl1) and same_bits(q.filter(), filt1) and sref.word(ctl1, sref.COUNT) == 2      # (3, 11) left, the new entry came
        # ---- the middle of a phase: p, n, zp, zn off the central path, a multiplier y
        if name in BIG:      # (the shared big case: the heavy lane of the 60 000 shape carries its weights)
            E = rref.big_entered(BIG[name])
            R, st_h, mu = {k: v.copy() for k, v in E["R"].items()}, E["state"], E["mu"]
        else:
            R, st_h, mu = rref.entered(P)
        zeta = math.sqrt(mu)
        R["blk"] = R1["blk"]
        z.upload(R)
        st = tuple(dev(a) for a in st_h)
        r_h = P["r"] if name in BIG else P["om"].jtprod(st_h[0], st_h[2])
        r = dev(r_h)
        # terms
        sigma, dcon, rhs = nan(n), nan(m), nan(S.n)
        z.call("terms", *map(_p, st), _p(r), _p(c), mu, zeta, _p(sigma), _p(dcon), _p(rhs))
        want = rref.terms(B, R, st_h, r_h, c_h, mu, zeta)
        assert same_bits(host(sigma, n), want[0]) and same_bits(host(dcon, m), want[1]) and same_bits(host(rhs, S.n), want[2])
        assert same_object(z.object(), R)      # terms writes nothing into the object
        # step
        sol_h = E["sol"] if name in BIG else rng.standard_normal(S.n)
        sol = dev(sol_h)
        dirs, alpha = tuple(nan(k) for k in S.dsizes), nan(2)
        z.call("step", *map(_p, st), _p(sol), mu, TAU, zeta, *map(_p, dirs), _p(alpha))
        poison = tuple(np.full(m, NAN) for _ in range(3))
        dirs_h, alpha_h, R = rref.step(B, R, st_h, sol_h, poison, mu, TAU, zeta)
        for t, w, k in zip(dirs, dirs_h, S.dsizes):
            assert same_bits(host(t, k), w)
        assert same_bits(host(alpha, 2), alpha_h) and 0.0 < alpha_h[0] <= 1.0 and 0.0 < alpha_h[1] <= 1.0
        assert same_object(z.object(), R)
        # a NaN in dy: alpha_primal is +0.0
        sol_bad = sol.clone()
        sol_bad[n + m // 2] = NAN
        alpha_bad = nan(2)
        dirs_bad = tuple(nan(k) for k in S.dsizes)
        z.call("step", *map(_p, st), _p(sol_bad), mu, TAU, zeta, *map(_p, dirs_bad), _p(alpha_bad))
        bad_h = sol_h.copy()
        bad_h[n + m // 2] = NAN
        _, want_bad, _ = rref.step(B, R, st_h, bad_h, poison, mu, TAU, zeta)
        assert same_bits(host(alpha_bad, 2), want_bad) and want_bad[0] == 0.0
        z.upload(R)      # (the poisoned call wrote its dp, dn into the object)
        # merit at the state
        m0 = nan(3)
        z.call("merit", 0, _p(st[0]), _p(st[1]), _p(c), zeta, _p(m0))
        m0_h = host(m0, 3)
        for _ in range(3):
            again = nan(3)
            z.call("merit", 0, _p(st[0]), _p(st[1]), _p(c), zeta, _p(again))
            assert same_bits(host(again, 3), m0_h)
        check_merit(S, R, 0, st_h[0], st_h[1], c_h, zeta, m0_h, f"{name} merit(0)")
        # begin: the slope and the inner block
        start = z.inner.block()
        assert sref.word(start, sref.STATUS) == sref.UNUSABLE
        z.call("begin", _p(st[0]), _p(st[1]), _p(sol), _p(dirs[0]), _p(m0), _p(alpha), mu, zeta)
        first = z.inner.block()
        for _ in range(3):
            z.call("begin", _p(st[0]), _p(st[1]), _p(sol), _p(dirs[0]), _p(m0), _p(alpha), mu, zeta)
            assert same_bits(z.inner.block(), first)
        slope = rref.slope(B, R, st_h, sol_h, dirs_h[0], mu, zeta, S.info["workgroups"])      # the restatement's, in the device's order
        print(name, f"begin: slope {float(first[sref.SLOPE])!r}, device order {float(slope)!r}")
        ref = rref.begin(start, slope, m0_h, alpha_h, mu)
        assert same_bits(first, ref) and sref.word(first, sref.STATUS) == sref.SEARCHING and first[sref.ALPHA] == alpha_h[0], (first, ref)
        assert same_bits(q.block(), ctl1)      # the ORIGINAL block is not the inner one
        # trial, merit at the trial point
        xt, s_t = nan(n), nan(m)
        z.call("trial", _p(st[0]), _p(st[1]), _p(sol), _p(dirs[0]), _p(xt), _p(s_t))
        xt_h, s_t_h, R = rref.trial(B, R, first, st_h[0], st_h[1], sol_h, dirs_h[0], (np.full(n, NAN), np.full(m, NAN)))
        assert same_bits(host(xt, n), xt_h) and same_bits(host(s_t, m), s_t_h) and same_object(z.object(), R)
        ct_h = c_h + 1e-3 * rng.standard_normal(m)
        ct, m1 = dev(ct_h), nan(3)
        z.call("merit", 1, _p(xt), _p(s_t), _p(ct), zeta, _p(m1))
        m1_h = host(m1, 3)
        check_merit(S, R, 1, xt_h, s_t_h, ct_h, zeta, m1_h, f"{name} merit(1)")
        # trial under FAILED and UNUSABLE: nothing is stored
        for status in (sref.FAILED, sref.UNUSABLE):
            blk = first.copy()
            sref.set_word(blk, sref.STATUS, status)
            z.inner.upload(blk, z.inner.filter())
            Rp = dict(R, pt=np.full(m, NAN), nt=np.full(m, NAN))
            z.upload(Rp)
            xt2, st2 = nan(n), nan(m)
            z.call("trial", _p(st[0]), _p(st[1]), _p(sol), _p(dirs[0]), _p(xt2), _p(st2))
            assert np.isnan(host(xt2, n)).all() and np.isnan(host(st2, m)).all() and same_object(z.object(), Rp)
        z.upload(R)
        # error
        out = nan(8)
        z.call("error", *map(_p, st), _p(r), _p(c), mu, zeta, _p(out))
        out_h = host(out, 8)
        again = nan(8)
        z.call("error", *map(_p, st), _p(r), _p(c), mu, zeta, _p(again))
        assert same_bits(host(again, 8), out_h)
        head, ay, mult, th, lg = rref.error(B, R, st_h, r_h, c_h, mu, zeta)
        assert same_bits(out_h[:4], head), (out_h[:4], head)
        sums = rref.error_sums(B, R, st_h, c_h, S.info["workgroups"])
        print(name, "error: out[4..7]", out_h[4:].tolist(), "device order", sums.tolist())
        assert same_bits(out_h[4:7], sums[:3]), (out_h[4:7], sums[:3])
        logs_within(float(out_h[7]), sums[3], lg, "L")
        assert same_bits(out_h[6:], m0_h[1:])      # theta_R and L: the bits of merit(0)
        z.call("error", *map(_p, st), None, _p(c), mu, zeta, _p(again))
        head_nr, *_ = rref.error(B, R, st_h, None, c_h, mu, zeta)
        assert np.isnan(host(again, 8)[0]) and same_bits(host(again, 8)[1:], np.concatenate([head_nr[1:], out_h[4:]]))
        # update: a zero step length moves nothing, then the step
        for pair in ([0.0, alpha_h[1]], [alpha_h[0], 0.0]):      # EITHER step length +0.0
            zero = dev(np.array(pair))
            z.call("update", *map(_p, st), _p(sol), *map(_p, dirs), _p(zero), mu, KAPPA)
            for t, w, k in zip(st, st_h, S.sizes):
                assert same_bits(host(t, k), w)
            assert same_object(z.object(), R)
        z.call("update", *map(_p, st), _p(sol), *map(_p, dirs), _p(alpha), mu, KAPPA)
        new_h, R = rref.update(B, R, st_h, sol_h, dirs_h, alpha_h, mu)
        for t, w, k in zip(st, new_h, S.sizes):
            assert same_bits(host(t, k), w)
        assert same_object(z.object(), R) and not same_bits(new_h[0], st_h[0])
        # leave: below the threshold only y moves; above it the present multipliers become 1.0
        for bump in (False, True):
            with np.errstate(invalid="ignore"):      # (the guarded multipliers of the step above reach 1e12: below the threshold first)
                cur = [np.minimum(a, 50.0) if k >= 3 else a.copy() for k, a in enumerate(new_h)]
            if bump and B["counts"]["nz"]:
                which, on = next((k, o) for k, o in ((3, B["hasL"]), (4, B["hasU"]), (5, B["gL"]), (6, B["gU"])) if o.any())
                cur[which][np.flatnonzero(on)[-1]] = 1000.5
            stl = tuple(dev(a) for a in cur)
            Ra = dict(R)
            Ra["blk"] = R["blk"].copy()
            Ra["blk"].view(np.int64)[0] = rref.RETURN
            z.upload(Ra)
            z.call("leave", *map(_p, stl[2:]))
            want_st, want_blk = rref.leave(B, Ra["blk"], tuple(cur))
            for t, w, k in zip(stl, want_st, S.sizes):
                assert same_bits(host(t, k), w)
            assert same_object(z.object(), dict(Ra, blk=want_blk))
            if bump and B["counts"]["nz"]:
                assert want_blk[rref.R_ZMAX] == 1000.5


@pytest.mark.parametrize("name", list(BIG))
def test_big_extremes_on_later_trips(name, built):
    """resto_step's two step lengths, resto_error's four maxima and resto_leave_max with their deciding value planted at each seam
    position of tests/test_gpu_barrier.py in turn: the slot carries the bits numpy gives for the planted entry, which beats the rest"""
    from test_gpu_barrier import cut_at, planted
    with layer(name) as S:
        P, B = S.P, S.B
        n, m = S.nvar, S.ncon
        big_facts(name, S)
        E = rref.big_entered(BIG[name])
        R, st_h, mu = E["R"], E["state"], E["mu"]
        zeta = math.sqrt(mu)
        q = S.search()
        z = S.resto(q)
        z.upload(R)
        st = tuple(dev(a) for a in st_h)
        r_h, c_h = P["r"], P["c"]
        r, c = dev(r_h), dev(c_h)
        sol_h = np.random.default_rng(43).standard_normal(S.n)      # (not the shared direction: its heavy lane leaves no room below its step lengths)
        sol = dev(sol_h)
        poison = tuple(np.full(m, NAN) for _ in range(3))
        base_alpha = rref.step(B, R, st_h, sol_h, poison, mu, TAU, zeta)[1]
        dirs, alpha = tuple(nan(k) for k in S.dsizes), nan(2)

        def cut_R(iv, ir):
            C1 = {k: R[k][ir] for k in rref.ROWS}
            C1.update({k: R[k][iv] for k in rref.VARS})
            C1["blk"] = R["blk"]
            return C1
        for slot, what in ((0, "alpha_primal"), (1, "alpha_dual")):
            for label, i in planted(S, "lower"):
                B1, st1, iv, ir = cut_at(S, st_h, i)
                value = -1e9 if slot == 0 else 1e9
                sol[i] = value
                z.call("step", *map(_p, st), _p(sol), mu, TAU, zeta, *map(_p, dirs), _p(alpha))
                got = host(alpha, 2)
                one = rref.step(B1, cut_R(iv, ir), st1, np.array([value]), tuple(np.full(len(ir), NAN) for _ in range(3)), mu, TAU, zeta)[1]
                print(f"{name} {what} planted at {label}: {got.tolist()}, the entry alone {one.tolist()}, the rest {base_alpha.tolist()}")
                assert one[slot] < base_alpha[slot] and same_bits(got, np.minimum(base_alpha, one)), (what, label, got, one)
                sol[i] = float(sol_h[i])
        # a NaN direction; a point exactly on its relaxed bound with a direction through it: alpha_primal = +0.0, update moves nothing
        import torch
        four = np.concatenate([R[k] for k in ("p", "n", "zp", "zn")])
        got_four = np.empty(4 * m)
        for label, i in planted(S, "lower"):
            j, vec = (i, 0) if i < n else (i - n, 1)
            bound = float((B["xl"] if i < n else B["rl"])[j])
            for case, value, x_value in (("NaN direction", NAN, None), ("on its bound", -1.0 if i < n else -1e9, bound)):
                B1, st1, iv, ir = cut_at(S, st_h, i)
                st1 = [a.copy() for a in st1]
                old = float(st[vec][j])
                if x_value is not None:
                    st[vec][j] = x_value
                    st1[vec][0] = x_value
                sol[i] = value
                z.call("step", *map(_p, st), _p(sol), mu, TAU, zeta, *map(_p, dirs), _p(alpha))
                got = host(alpha, 2)
                one = rref.step(B1, cut_R(iv, ir), tuple(st1), np.array([value]), tuple(np.full(len(ir), NAN) for _ in range(3)), mu, TAU, zeta)[1]
                print(f"{name} {case} at {label}: alpha {got.tolist()}")
                assert same_bits(got[:1], [0.0]) and same_bits(got, np.minimum(base_alpha, one)), (case, label, got, one)
                before = [t.clone() for t in st]
                z.call("update", *map(_p, st), _p(sol), *map(_p, dirs), _p(alpha), mu, KAPPA)
                assert all(torch.equal(a.view(torch.int64), b_.view(torch.int64)) for a, b_ in zip(st, before)), (case, label)
                z.q._copy(got_four.ctypes.data, z.d_vec, got_four.nbytes, 2)
                assert same_bits(got_four, four), (case, label)
                sol[i] = float(sol_h[i])
                st[vec][j] = old
        # the four maxima: r (a variable), y (a row), c (a row), a multiplier (an entry with a lower bound)
        base = rref.error(B, R, st_h, r_h, c_h, mu, zeta)[0]
        out = nan(8)

        def error_head():
            z.call("error", *map(_p, st), _p(r), _p(c), mu, zeta, _p(out))
            return host(out, 8)[:4]
        assert same_bits(error_head(), base)
        for slot, what, kind in ((0, "r", "variable"), (1, "y", "row"), (2, "c", "row"), (3, "z", "lower")):
            for label, i in planted(S, kind):
                B1, st1, iv, ir = cut_at(S, st_h, i)
                st1 = [a.copy() for a in st1]
                r1, c1 = r_h[iv].copy(), c_h[ir].copy()
                j = i if i < n else i - n
                vec, host_vec = {"r": (r, r1), "y": (st[2], st1[2]), "c": (c, c1), "z": (st[3], st1[3]) if i < n else (st[5], st1[5])}[what]
                old = float(vec[j])
                vec[j] = 1e30
                host_vec[0] = 1e30
                got = error_head()
                one = rref.error(B1, cut_R(iv, ir), tuple(st1), r1 if len(iv) else None, c1, mu, zeta)[0]
                want = np.maximum(base, np.where(np.isnan(one), 0.0, one))      # (a cut without variables has no out[0])
                print(f"{name} out[{slot}] planted ({what}) at {label}: {got.tolist()}")
                assert one[slot] > base[slot] and same_bits(got, want), (what, label, got, want)
                vec[j] = old
        assert same_bits(error_head(), base)
        # resto_leave_max: every present multiplier at most 50 but the planted one, below the reset threshold: nothing but y moves
        with np.errstate(invalid="ignore"):
            cur = [np.minimum(a, 50.0) if k >= 3 else a.copy() for k, a in enumerate(st_h)]
        stl = tuple(dev(a) for a in cur)
        active = R["blk"].copy()
        active.view(np.int64)[0] = rref.RETURN
        got_blk = np.empty(8)
        for label, i in planted(S, "upper"):
            j = i if i < n else i - n
            vec = stl[4] if i < n else stl[6]
            vec[j] = 777.25
            z.q._copy(z.d_blk, active.ctypes.data, 64, 1)
            z.call("leave", *map(_p, stl[2:]))
            z.q._copy(got_blk.ctypes.data, z.d_blk, 64, 2)
            print(f"{name} leave_max planted at {label}: {got_blk[rref.R_ZMAX]}")
            assert same_bits(got_blk[rref.R_ZMAX], 777.25) and int(got_blk.view(np.int64)[0]) == rref.NONE, (label, got_blk)
            assert float(vec[j]) == 777.25      # below the threshold: the multipliers stay
            vec[j] = 50.0
        z.q._copy(z.d_blk, active.ctypes.data, 64, 1)
        z.call("leave", *map(_p, stl[2:]))
        z.q._copy(got_blk.ctypes.data, z.d_blk, 64, 2)
        assert same_bits(got_blk[rref.R_ZMAX], 50.0)


def test_the_return_test_and_the_filter_append(built):
    """the tables of tests/resto_reference.py: the object's block after check; the ORIGINAL block and filter after enter"""
    with layer("wb_eq") as S:
        q = S.search()
        z = S.resto(q)
        R = z.object()
        for name, blk, ctl_o, filt_o, f, mer, mu, want in rref.check_cases(q.cap):
            q.upload(ctl_o, filt_o)
            z.upload(dict(R, blk=blk))
            tf, tm = dev([f]), dev(mer)
            z.call("check", _p(tf), _p(tm), mu)
            got = z.object()["blk"]
            ref = rref.check(blk, ctl_o, filt_o, f, mer, mu, cap=q.cap)
            assert same_bits(got, ref) and int(got.view(np.int64)[0]) == want, name
            assert same_bits(q.block(), ctl_o) and same_bits(q.filter(), filt_o), name      # check writes nothing into the search
        P, B = S.P, S.B
        for name, ctl_o, filt_o, count, overflow in rref.append_cases(q.cap):
            q.upload(ctl_o, filt_o)
            z.upload(R)
            st = tuple(dev(a) for a in P["state"])
            tc = dev(P["c"])
            z.call("enter", *map(_p, st), _p(tc), 1.0)
            blk, ctl, filt = rref.enter_filter(R["blk"], ctl_o, filt_o, q.opts)
            assert same_bits(q.block(), ctl) and same_bits(q.filter(), filt) and same_bits(z.object()["blk"], blk), name
            assert sref.word(ctl, sref.COUNT) == count and bool(sref.word(ctl, sref.FLAGS) & 2) == overflow, name


def test_refusals(built):
    from infiniteexamodels.jl_amd import lib as iemlib
    with layer("wb_ineq") as S:
        L = S.L
        err = lambda: L.iem_last_error().decode()
        q = S.search()
        out = C.c_void_p()
        for bad, word in ((dict(rho=0.0), "rho"), (dict(rho=-1.0), "rho"), (dict(rho=NAN), "rho"), (dict(kappa_resto=0.0), "kappa_resto"), (dict(kappa_resto=1.0), "kappa_resto"),
                          (dict(bound_mult_reset_threshold=-1.0), "threshold")):
            o = iemlib.RestoOpts.defaults(**bad)
            assert L.iem_resto_create(q.s, C.byref(o), C.byref(out)) == -4 and word in err() and not out.value, bad
        o = iemlib.RestoOpts.defaults()
        o.struct_size = 4
        assert L.iem_resto_create(q.s, C.byref(o), C.byref(out)) == -4 and "struct_size" in err()
        assert L.iem_resto_create(q.s, None, None) == -4 and "null" in err()
        z = S.resto(q)
        st = tuple(dev(a) for a in S.P["state"])
        c, sol, a2, o3, o8 = dev(S.P["c"]), nan(S.n), nan(2), nan(3), nan(8)
        dirs = tuple(nan(k) for k in S.dsizes)
        p = list(map(_p, st))
        assert L.iem_resto_enter(z.z, *p, _p(c), -1.0) == -4 and "mu" in err()
        assert L.iem_resto_enter(z.z, *p, None, 1.0) == -4 and "null" in err()
        assert L.iem_resto_enter(z.z, p[0], None, *p[2:], _p(c), 1.0) == -4 and "null" in err()      # s with inequality rows
        assert L.iem_resto_terms(z.z, *p, _p(nan(S.nvar)), _p(c), 0.1, -1.0, _p(nan(S.nvar)), _p(nan(S.ncon)), _p(nan(S.n))) == -4 and "zeta" in err()
        assert L.iem_resto_terms(z.z, *p, None, _p(c), 0.1, 0.3, _p(nan(S.nvar)), _p(nan(S.ncon)), _p(nan(S.n))) == -4 and "null" in err()
        assert L.iem_resto_step(z.z, *p, _p(sol), 0.1, 0.0, 0.3, *map(_p, dirs), _p(a2)) == -4 and "tau" in err()
        assert L.iem_resto_step(z.z, *p, _p(sol), 0.1, 0.99, 0.3, *map(_p, dirs), None) == -4 and "null" in err()
        assert L.iem_resto_merit(z.z, 3, p[0], p[1], _p(c), 0.3, _p(o3)) == -4 and "which" in err()
        assert L.iem_resto_merit(z.z, 1, p[0], p[1], _p(c), 0.3, None) == -4 and "null" in err()
        assert L.iem_resto_begin(z.z, p[0], p[1], _p(sol), _p(dirs[0]), None, _p(a2), 0.1, 0.3) == -4 and "null" in err()
        assert L.iem_resto_trial(z.z, p[0], p[1], _p(sol), _p(dirs[0]), None, _p(nan(S.ncon))) == -4 and "null" in err()
        assert L.iem_resto_update(z.z, *p, _p(sol), *map(_p, dirs), _p(a2), 0.1, 0.5) == -4 and "kappa_sigma" in err()
        assert L.iem_resto_error(z.z, *p, None, None, 0.1, 0.3, _p(o8)) == -4 and "null" in err()
        assert L.iem_resto_check(z.z, None, _p(a2), 0.1) == -4 and "null" in err()
        assert L.iem_resto_leave(z.z, None, *p[3:]) == -4 and "null" in err()
        assert np.isnan(host(o8, 8)).all() and np.isnan(host(o3, 3)).all() and np.isnan(host(a2, 2)).all()      # refused before any device work
        v = iemlib.RestoState()
        v.struct_size = 4
        assert L.iem_resto_state(z.z, C.byref(v)) == -4 and "struct_size" in err()
        v.struct_size = C.sizeof(iemlib.RestoState)
        assert L.iem_resto_state(z.z, C.byref(v)) == 0 and (v.state, v.theta_start) == (rref.NONE, 0.0)


def test_one_iteration_in_one_graph(built):
    """eval_residual(0); error; jac_hess_coord(0); terms; assemble; factor; refined solve; step; merit(0); begin; 6 × {trial, cons,
    merit(1), accept}; update; obj; cons; barrier_merit; check — on wb_eq, entered at the shared state: eager, then captured once and
    replayed twice from the same start: bitwise the eager run, the object, the inner block and the state included"""
    import torch
    from infiniteexamodels.jl_amd.barrier import BarrierLayer, FilterSearch, Restoration
    from infiniteexamodels.jl_amd.kkt_chain import KKTObject
    from infiniteexamodels.jl_amd.model import ExaModel
    P = rref.point("wb_eq")
    B = P["B"]
    gm = ExaModel(P["core"], device=0, blob=P["blob"])
    n, m = P["om"].nvar, P["om"].ncon
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    new = lambda k: torch.full((k,), NAN, dtype=torch.float64, device="cuda")
    try:
        with BarrierLayer(gm) as bar, KKTObject(gm) as kkt, FilterSearch(bar) as fs, Restoration(fs) as resto:
            state = tuple(T(np.where(np.isnan(a), 0.0, a)) for a in P["state"])
            x, s, y = state[0], state[1], state[2]
            c, r, f = new(m), new(n), new(1)
            jv, hv = new(int(gm.meta.nnzj)), new(int(gm.meta.nnzh))
            sigma, dcon, rhs, sol = new(n), new(m), new(n + m), new(n + m)
            dirs, alpha = (torch.zeros(m, dtype=torch.float64, device="cuda"), new(n), new(n), torch.zeros(m, dtype=torch.float64, device="cuda"),
                           torch.zeros(m, dtype=torch.float64, device="cuda")), new(2)
            xt, st, ct, m3, mt3, m2, e8 = new(n), torch.zeros(m, dtype=torch.float64, device="cuda"), new(m), new(3), new(3), new(2), new(8)
            inertia = torch.zeros(3, dtype=torch.int64, device="cuda")
            gm.cons(x, c)
            with np.errstate(invalid="ignore"):
                mu = max(0.1, float(np.abs(rref.infeasibility(B, P["om"].cons(P["state"][0]), P["state"][1])).max()))
            zeta = math.sqrt(mu)
            resto.enter(state, c, mu)
            torch.cuda.synchronize()
            ptr = resto.device()
            inner_ctl, _ = resto.inner.device()
            start_state = [t.clone() for t in state]
            nbytes = (12 * m + 2 * n) * 8
            vec0, blk0, ctl0 = np.empty(12 * m + 2 * n), np.empty(8), np.empty(16)
            assert hip().hipMemcpy(vec0.ctypes.data, ptr["p"], nbytes, 2) == 0 and hip().hipMemcpy(blk0.ctypes.data, ptr["block"], 64, 2) == 0
            assert hip().hipMemcpy(ctl0.ctypes.data, inner_ctl, 128, 2) == 0
            assert int(blk0.view(np.int64)[0]) == rref.ACTIVE
            L, k = kkt._handle()

            def load():
                torch.cuda.synchronize()
                for t, a in zip(state, start_state):
                    t.copy_(a)
                assert hip().hipMemcpy(ptr["p"], vec0.ctypes.data, nbytes, 1) == 0 and hip().hipMemcpy(ptr["block"], blk0.ctypes.data, 64, 1) == 0
                assert hip().hipMemcpy(inner_ctl, ctl0.ctypes.data, 128, 1) == 0
                for t in (c, r, f, sigma, dcon, rhs, sol, alpha, xt, ct, m3, mt3, m2, e8, dirs[1], dirs[2]):
                    t.fill_(NAN)
                torch.cuda.synchronize()

            def iteration():
                gm.eval_residual(x, y, 0.0, c=c, out=r, obj=f)
                resto.error(state, r, c, mu, zeta, out=e8)
                gm.jac_hess_coord(x, y, jv, hv, obj_weight=0.0)
                resto.terms(state, r, c, mu, zeta, out=(sigma, dcon, rhs))
                kkt.assemble(hv, jv, sigma, 0.0, DELTA_C, dcon=dcon, at=(x, y, 0.0))
                S_check(L.iem_kkt_factor_async(k, _p(inertia)))
                S_check(L.iem_kkt_solve_refined_diag(k, _p(x), _p(y), 0.0, _p(sigma), _p(dcon), 0.0, DELTA_C, 1, _p(rhs), n + m, _p(sol), n + m, 1, None))
                resto.step(state, sol, mu, TAU, zeta, out=dirs, alpha=alpha)
                resto.merit(0, x, s, c, zeta, out=m3)
                resto.begin(state, sol, dirs[0], m3, alpha, mu, zeta)
                for _ in range(6):
                    resto.trial(state, sol, dirs[0], xt, st)
                    gm.cons(xt, ct)
                    resto.merit(1, xt, st, ct, zeta, out=mt3)
                    resto.inner.accept(mt3[0:1], mt3[1:3], mu, alpha)
                resto.update(state, sol, dirs, alpha, mu)
                gm.obj_device(x, out=f)
                gm.cons(x, c)
                bar.merit(x, s, c, out=m2)
                resto.check(f, m2, 0.1)

            from infiniteexamodels.jl_amd import lib as iemlib
            S_check = iemlib.check

            def results():
                torch.cuda.synchronize()
                vec, blk, ctl = np.empty(12 * m + 2 * n), np.empty(8), np.empty(16)
                assert hip().hipMemcpy(vec.ctypes.data, ptr["p"], nbytes, 2) == 0 and hip().hipMemcpy(blk.ctypes.data, ptr["block"], 64, 2) == 0
                assert hip().hipMemcpy(ctl.ctypes.data, inner_ctl, 128, 2) == 0
                return [t.clone() for t in state + (c, r, f, sigma, dcon, rhs, sol, alpha, xt, ct, m3, mt3, m2, e8) + dirs], vec, blk, ctl, inertia.clone()
            load()
            iteration()
            eager = results()
            E = eager[0]
            print("wb_eq iteration: inertia", eager[4].tolist(), "inner status", sref.word(eager[3], sref.STATUS), "alpha", E[14].tolist(), "state", int(eager[2].view(np.int64)[0]),
                  "theta", eager[2][rref.R_THETA], "theta_R", eager[3][sref.THETA0], "->", eager[3][sref.THETA_T])
            assert eager[4].tolist()[1:] == [m, 0]
            assert sref.word(eager[3], sref.STATUS) in (sref.F_TYPE, sref.H_TYPE) and float(E[14][0]) > 0.0
            assert not torch.equal(E[0], start_state[0]) and np.isfinite(eager[1]).all() and math.isfinite(eager[2][rref.R_THETA])
            # the device's step against the restatement, from the device's solve
            R = {kk: vec0[i * m:(i + 1) * m] for i, kk in enumerate(rref.ROWS)}
            R.update({kk: vec0[12 * m + i * n:12 * m + (i + 1) * n] for i, kk in enumerate(rref.VARS)})
            st_h = tuple(a.cpu().numpy() for a in start_state)
            keep = tuple(np.zeros(m) for _ in range(3))
            dirs_h, alpha_h, R = rref.step(B, R, st_h, E[13].cpu().numpy(), keep, mu, TAU, zeta)
            new_h, R = rref.update(B, R, st_h, E[13].cpu().numpy(), dirs_h, E[14].cpu().numpy(), mu)
            for got, want in zip(E[:7], new_h):
                assert same_bits(got.cpu().numpy(), want)
            assert same_bits(eager[1][:4 * m], np.concatenate([R[kk] for kk in ("p", "n", "zp", "zn")]))
            load()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                gm._sync_stream()
                iteration()
            gm._sync_stream()
            for _ in range(2):
                load()
                graph.replay()
                again = results()
                for a, b in zip(again[0], eager[0]):
                    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
                assert same_bits(again[1], eager[1]) and same_bits(again[2], eager[2]) and same_bits(again[3], eager[3]) and torch.equal(again[4], eager[4])
    finally:
        gm.close()


@pytest.mark.parametrize("name", list(rref.WB_MODELS))
def test_the_loop_needs_the_phase(name, built):
    """tests/resto_loop.py with the device objects: FAILED without the phase, the optimum with it"""
    import resto_loop
    from infiniteexamodels.jl_amd.model import ExaModel
    core = rref.wb_core(name)
    gm = ExaModel(core, device=0, blob=core.to_blob())
    try:
        without = resto_loop.solve(gm, max_restorations=0)
        got = resto_loop.solve(gm)
    finally:
        gm.close()
    show = lambda o: {k: o[k] for k in ("status", "iterations", "error", "objective", "restorations", "resto_iterations", "trials", "failed", "why")}
    print(name, "without:", show(without))
    print(name, "with:   ", show(got))
    assert without["status"] == "search failed" and without["statuses"].get("failed", 0) >= 1 and without["restorations"] == 0
    optimum = rref.WB_MODELS[name]["optimum"]
    assert got["status"] == "solved" and got["restorations"] >= 1 and got["error"] <= 1e-8
    assert abs(got["objective"] / optimum - 1.0) <= 1e-6
