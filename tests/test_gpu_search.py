"""The filter line search (iem_search_*, csrc/iem_search_device.h) on the MI355X.

BITWISE against tests/search_reference.py (the numpy restatement, no tolerance): the WHOLE control block after begin — the slope
word included: search_reference.slope restates the parked sum in the device's order (barrier_reference.device_sum) on the object's
own grid of info["workgroups"] workgroups, and nothing of the device's is fed into the restatement — the trial point, and — for
every hand-built case of the acceptance table — the block, the filter (entries, order, count) and d_alpha[0] after accept.  The
slope repeats bit for bit over ten calls.  Outputs go into NaN-poisoned buffers with NaN padding; entries of s, ds on equality rows
are NaN on the way in, those of st still NaN afterwards.

Models: those of tests/test_gpu_barrier.py — pandemic_100x7 has 47 workgroups, more than one ticket group of 32 — and its two big
shapes, quadrotor(27 000) and quadrotor(60 000) of barrier_reference.big_point (4096 workgroups, two and three trips of the stride
loop, the nvar seam inside the second trip of the larger; asserted and printed): begin (the whole block), trial, and one accept on
the resulting words, bit for bit.

THE LADDER.  The direction is the Newton direction of the shared state (host solve of the condensed system, delta_w = 1e-2), the
step lengths are those of the restated barrier_step.  opf_7 as it is: the first rung (alpha_max = 1.6e-8) raises phi by 0.18 and does
not lower theta by a factor 1 − 1e-5 — rejected on finite numbers — and the second lowers phi by 0.13 — h-type.  pandemic_20x3 with
the direction (sol, ds and the multiplier directions) times 4: the rungs at 4 and 2 times the fraction-to-the-boundary step leave the
interior (phi_t is NaN), the third is the unscaled step and is accepted, h-type by theta (1217 against 1273).  The test checks both
patterns on the reference side.  Times 4 on both models and max_trials = 2: a search that fails."""
import contextlib
import ctypes as C
import math
import types

import numpy as np
import pytest

import barrier_reference as bref
import kkt_diag_reference as dref
import search_reference as sref
from barrier_reference import KAPPA, MU
from test_gpu_barrier import BIG, big_facts, point

pytestmark = pytest.mark.gpu
MODELS = ["opf_7", "farmer_5", "pandemic_20x3", "quadrotor_100", "pandemic_100x7"]
LADDER = {"opf_7": 1.0, "pandemic_20x3": 4.0}      # the factor on the direction (module docstring)
RUNGS = 4
PAD = 5
DW, DC = 1e-2, 1e-6
NAN = float("nan")
SIGMA = 1.0


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def nan(n):
    import torch
    return torch.full((n + PAD,), NAN, dtype=torch.float64, device="cuda")


def dev(a):
    """a host vector at the head of a NaN-poisoned buffer with PAD entries behind it"""
    import torch
    buf = nan(len(a))
    buf[:len(a)] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    return buf


def host(buf, n):
    assert bool(np.isnan(buf[n:].cpu().numpy()).all()), "padding touched"
    return buf[:n].cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


_hip = []


def hip():
    """the HIP runtime of this process (the one torch loaded), for copies to and from the object's own device memory"""
    if not _hip:
        path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
        rt = C.CDLL(path)
        rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        rt.hipMemcpy.restype = C.c_int
        _hip.append(rt)
    return _hip[0]


class Search:
    """the raw search object of a layer: create / destroy, and the block and the filter read and written through hipMemcpy"""

    def __init__(self, S, **opts):
        from infiniteexamodels.jl_amd import lib as iemlib
        self.S, self.opts = S, dict(sref.OPTS, **opts)
        self.o = iemlib.SearchOpts.defaults(**opts)
        self.s = C.c_void_p()
        S.check(S.L.iem_search_create(S.b, C.byref(self.o), C.byref(self.s)))
        ctl, flt = C.c_void_p(), C.c_void_p()
        S.check(S.L.iem_search_device(self.s, C.byref(ctl), C.byref(flt)))
        self.ctl, self.flt, self.cap = ctl.value, flt.value, int(self.opts["filter_capacity"])
        assert self.ctl and self.flt

    def _copy(self, dst, src, nbytes, kind):
        import torch
        torch.cuda.synchronize()
        assert hip().hipMemcpy(dst, src, nbytes, kind) == 0

    def block(self):
        out = np.empty(16)
        self._copy(out.ctypes.data, self.ctl, 128, 2)
        return out

    def filter(self):
        out = np.empty((self.cap, 2))
        self._copy(out.ctypes.data, self.flt, self.cap * 16, 2)
        return out

    def upload(self, ctl, filt):
        ctl, filt = np.ascontiguousarray(ctl, dtype=np.float64), np.ascontiguousarray(filt, dtype=np.float64)
        assert ctl.shape == (16,) and filt.shape == (self.cap, 2)
        self._copy(self.ctl, ctl.ctypes.data, 128, 1)
        self._copy(self.flt, filt.ctypes.data, self.cap * 16, 1)

    def begin(self, x, s, g, sol, ds, obj, err, alpha, mu=MU, sigma=SIGMA):
        self.S.check(self.S.L.iem_search_begin(self.s, _p(x), _p(s), _p(g), _p(sol), _p(ds), _p(obj), _p(err), _p(alpha), mu, sigma))

    def trial(self, x, s, sol, ds, xt, st):
        self.S.check(self.S.L.iem_search_trial(self.s, _p(x), _p(s), _p(sol), _p(ds), _p(xt), _p(st)))

    def accept(self, ft, merit, alpha, mu=MU, sigma=SIGMA):
        self.S.check(self.S.L.iem_search_accept(self.s, _p(ft), _p(merit), mu, sigma, _p(alpha)))

    def close(self):
        if self.s is not None:
            self.S.check(self.S.L.iem_search_destroy(self.s))
            self.s = None


@contextlib.contextmanager
def layer(name, seed=0):
    """the model handle, the raw barrier object and the shared point (tests/test_gpu_barrier.py's; a big shape: on the point's own
    bounds)"""
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.model import ExaModel
    P = point(name, seed)
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
        gm._sync_stream()
        yield S
    finally:
        for q in made:
            q.close()
        iemlib.check(gm._L.iem_barrier_destroy(b))
        gm.close()


def inputs(S, seed=0):
    """host side of a search at the shared point: grad f from the oracle, a random direction with NaN in ds on equality rows (never
    read), f, and a step length pair"""
    P, B = S.P, S.B
    rng = np.random.default_rng(77 + seed)
    g = P["om"].grad(P["state"][0])
    sol = rng.standard_normal(S.n)
    ds = np.where(B["eq"], NAN, rng.standard_normal(S.ncon))
    return g, sol, ds, float(P["om"].obj(P["state"][0])), np.array([0.75, 0.5])


def device_error(S, st, r, c, mu=MU):
    out = nan(8)
    S.check(S.L.iem_barrier_error(S.b, *map(_p, st), _p(r), _p(c), mu, _p(out)))
    return out


@pytest.mark.parametrize("name", MODELS)
def test_slope_and_begin(name, built):
    with layer(name) as S:
        P, B = S.P, S.B
        x_h, s_h = P["state"][:2]
        g_h, sol_h, ds_h, f_h, alpha_h = inputs(S)
        st = tuple(dev(a) for a in P["state"])
        g, sol, ds, obj, alpha = dev(g_h), dev(sol_h), dev(ds_h), dev([f_h]), dev(alpha_h)
        err = device_error(S, st, dev(P["r"]), dev(P["c"]))
        err_h = host(err, 8)
        q = S.search()
        start = q.block()
        assert sref.word(start, sref.STATUS) == sref.UNUSABLE and not start[:9].any() and not start.view(np.int64)[10:].any()
        q.begin(st[0], st[1], g, sol, ds, obj, err, alpha)
        first = q.block()
        for _ in range(10):
            q.begin(st[0], st[1], g, sol, ds, obj, err, alpha)
            assert same_bits(q.block(), first)      # (a second begin keeps theta_min / theta_max: flag bit 0 is set)
        n_wg = S.info["workgroups"]
        slope = float(sref.slope(B, x_h, s_h, g_h, sol_h, ds_h, MU, SIGMA, n_wg))      # the restatement's, in the device's order: nothing of the device's
        terms = sref.slope_terms(B, x_h, s_h, g_h, sol_h, np.where(B["eq"], 0.0, ds_h), MU, SIGMA)
        print(name, f"slope {float(first[sref.SLOPE])!r}, device order {slope!r}, fsum {math.fsum(terms)!r}, terms {len(terms)}, workgroups {n_wg}")
        if name == "pandemic_100x7":
            assert n_wg == 47
        ref = sref.begin(start, slope, f_h, err_h, alpha_h, MU, SIGMA)
        assert same_bits(first, ref), (first, ref)
        assert sref.word(first, sref.STATUS) == sref.SEARCHING and float(first[sref.ALPHA]) == 0.75
        # another theta0 at a later point: theta_min / theta_max stay, the rest follows
        err2_h = err_h.copy(); err2_h[6] *= 3.0
        q.begin(st[0], st[1], g, sol, ds, obj, dev(err2_h), alpha)
        second = q.block()
        assert same_bits(second, sref.begin(first, slope, f_h, err2_h, alpha_h, MU, SIGMA)) and same_bits(second[5:7], first[5:7])
        # unusable: a step length of +0.0, a NaN in dx
        q.begin(st[0], st[1], g, sol, ds, obj, err, dev([0.0, 0.5]))
        blk = q.block()
        assert sref.word(blk, sref.STATUS) == sref.UNUSABLE and same_bits(blk, sref.begin(second, slope, f_h, err_h, [0.0, 0.5], MU, SIGMA))
        bad = sol_h.copy(); bad[S.nvar // 2] = NAN
        q.begin(st[0], st[1], g, dev(bad), ds, obj, err, alpha)
        blk = q.block()
        assert sref.word(blk, sref.STATUS) == sref.UNUSABLE and math.isnan(blk[sref.SLOPE]) and same_bits(blk[:1], [0.0]) and blk[sref.ALPHA_MAX] == 0.75
        # the filter was never touched, nor the inputs
        assert same_bits(host(alpha, 2), alpha_h) and same_bits(host(sol, S.n), sol_h)
        if B["counts"]["nz"] == 0:      # no bounds: the slope is the sum of sigma·g·dx
            assert np.array_equal(terms, (SIGMA * g_h) * sol_h[:S.nvar])


@pytest.mark.parametrize("name", ["opf_7", "farmer_5", "quadrotor_100", "pandemic_100x7"])
def test_trial(name, built):
    with layer(name) as S:
        P, B = S.P, S.B
        x_h, s_h = P["state"][:2]
        g_h, sol_h, ds_h, f_h, alpha_h = inputs(S)
        x, s, sol, ds = dev(x_h), dev(s_h), dev(sol_h), dev(ds_h)
        q = S.search()
        empty = np.full((q.cap, 2), NAN)
        poison = (np.full(S.nvar, NAN), np.full(S.ncon, NAN))
        for status, a in ((sref.SEARCHING, 0.375), (sref.H_TYPE, 1.0 / 3.0), (sref.F_TYPE, 1e-9), (sref.FAILED, 0.5), (sref.UNUSABLE, 0.5)):
            ctl = sref.block(alpha=a, alpha_max=1.0, status=status)
            q.upload(ctl, empty)
            xt, st = nan(S.nvar), nan(S.ncon)
            q.trial(x, s, sol, ds, xt, st)
            want = sref.trial(B, ctl, x_h, s_h, sol_h, ds_h, poison)
            got = host(xt, S.nvar), host(st, S.ncon)
            assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), status
            if status in (sref.FAILED, sref.UNUSABLE):
                assert np.isnan(got[0]).all() and np.isnan(got[1]).all()
            else:
                assert same_bits(got[0], x_h + a * sol_h[:S.nvar]) and np.isnan(got[1][B["eq"]]).all() and not np.isnan(got[1][~B["eq"]]).any()
            assert same_bits(q.block(), ctl)


@pytest.mark.parametrize("name", list(BIG))
def test_big_shapes_bitwise(name, built):
    """begin (the whole block), trial and one accept on the resulting words where the stride loop runs more than once"""
    with layer(name) as S:
        P, B = S.P, S.B
        big_facts(name, S)
        x_h, s_h = P["state"][:2]
        g_h, sol_h, ds_h, f_h, alpha_h = sref.big_inputs(BIG[name])
        err_h = np.array([0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.4, -3.0])
        x, s, g, sol, ds, obj, err, alpha = (dev(a) for a in (x_h, s_h, g_h, sol_h, ds_h, [f_h], err_h, alpha_h))
        q = S.search()
        start = q.block()
        q.begin(x, s, g, sol, ds, obj, err, alpha)
        first = q.block()
        q.begin(x, s, g, sol, ds, obj, err, alpha)
        ref = sref.begin(start, sref.slope(B, x_h, s_h, g_h, sol_h, ds_h, MU, SIGMA, S.info["workgroups"]), f_h, err_h, alpha_h, MU, SIGMA)
        print(name, "slope", repr(float(first[sref.SLOPE])), "restated", repr(float(ref[sref.SLOPE])))
        assert same_bits(first, ref), (first, ref)
        assert same_bits(q.block(), first) and sref.word(first, sref.STATUS) == sref.SEARCHING and float(first[sref.ALPHA]) == 0.75
        xt, st = nan(S.nvar), nan(S.ncon)
        q.trial(x, s, sol, ds, xt, st)
        want = sref.trial(B, first, x_h, s_h, sol_h, ds_h, (np.full(S.nvar, NAN), np.full(S.ncon, NAN)))
        got = host(xt, S.nvar), host(st, S.ncon)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
        assert np.isnan(got[1][B["eq"]]).all() and not np.isnan(got[1][~B["eq"]]).any() and not np.isnan(got[0]).any()
        assert same_bits(host(x, S.nvar), x_h) and same_bits(host(sol, S.n), sol_h)
        a = dev([NAN, 0.5])
        ft, merit = 1.5, np.array([0.3, -7.0])
        filt = q.filter()
        q.accept(dev([ft]), dev(merit), a)
        want_ctl, want_filt, want_alpha = sref.accept(first, filt, ft, merit, MU, SIGMA, q.opts)
        assert same_bits(q.block(), want_ctl) and same_bits(q.filter(), want_filt) and same_bits(host(a, 2), [want_alpha, 0.5]), (q.block(), want_ctl)
        assert sref.word(want_ctl, sref.STATUS) != sref.UNUSABLE


def _accept_cases():
    out = [(64, c) for c in sref.cases(64)]
    for cap in (64, 100):
        for k in sref.filter_sizes(cap):
            out += [(cap, c) for c in sref.sized_case(k, cap)]
    return out


def test_accept_table(built):
    """every case of the table of tests/test_search.py, uploaded as block + filter: the block, the whole filter and d_alpha[0]
    afterwards are the restatement's bits; filters of 0, 1, 63, 64, 65 and filter_capacity (64, 100) entries"""
    with layer("farmer_5") as S:
        searches = {}
        for cap, (name, ctl, filt, ft, merit, mu, sigma, o, _) in _accept_cases():
            if (cap, o["max_trials"]) not in searches:
                searches[cap, o["max_trials"]] = S.search(filter_capacity=cap, max_trials=o["max_trials"])
            q = searches[cap, o["max_trials"]]
            q.upload(ctl, filt)
            alpha = dev([NAN, 0.625])
            q.accept(dev([ft]), dev(merit), alpha, mu, sigma)
            want_ctl, want_filt, want_alpha = sref.accept(ctl, filt, ft, merit, mu, sigma, o)
            got_ctl, got_filt, got_alpha = q.block(), q.filter(), host(alpha, 2)
            assert same_bits(got_ctl, want_ctl), (name, got_ctl, want_ctl)
            assert same_bits(got_filt, want_filt), name
            assert same_bits(got_alpha, [want_alpha, 0.625]), (name, got_alpha)
            # a second accept on the result: decided or not, it is the restatement's again
            q.accept(dev([ft]), dev(merit), alpha, mu, sigma)
            again = sref.accept(want_ctl, want_filt, ft, merit, mu, sigma, o)
            assert same_bits(q.block(), again[0]) and same_bits(q.filter(), again[1]) and same_bits(host(alpha, 2), [again[2], 0.625]), name
        # reset: the filter emptied, the flags cleared, nothing else
        q = searches[64, 30]
        before = q.block()
        S.check(S.L.iem_search_reset(q.s))
        after = q.block()
        want = before.copy(); sref.set_word(want, sref.COUNT, 0); sref.set_word(want, sref.FLAGS, 0)
        assert same_bits(after, want) and sref.word(before, sref.COUNT) > 0


def newton_direction(P, factor):
    """``(sol, dirs, alpha)`` on the host: the Newton direction of the shared state and the restated barrier_step, all times `factor`"""
    from scipy.sparse.linalg import splu
    B, om, st = P["B"], P["om"], P["state"]
    sg, dcn, rh = bref.terms(B, st, P["r"], P["c"])
    K = dref.host_kkt_diag(om, st[0], st[2], sg, DW, dcn + DC)
    sol = splu(K.tocsc()).solve(rh)
    dirs, alpha = bref.step(B, st, sol, tuple(np.full(om.ncon, NAN) for _ in range(3)))
    return sol * factor, tuple(d * factor for d in dirs), alpha


def _ladder(S, q, st, bufs, rungs=RUNGS):
    g, sol, dirs, obj, err, alpha, xt, st_t, fts, cts, ms, r, c, out = bufs
    S.gm._sync_stream()      # (the handle runs on torch's current stream: the capturing one inside a capture)
    q.begin(st[0], st[1], g, sol, dirs[0], obj, err, alpha)
    for k in range(rungs):
        q.trial(st[0], st[1], sol, dirs[0], xt, st_t)
        S.gm.obj_device(xt[:S.nvar], out=fts[k])
        S.gm.cons(xt[:S.nvar], cts[k][:S.ncon])
        S.gm._sync_stream()
        S.check(S.L.iem_barrier_merit(S.b, _p(xt), _p(st_t), _p(cts[k]), _p(ms[k])))
        q.accept(fts[k], ms[k], alpha)
    S.check(S.L.iem_barrier_update(S.b, *map(_p, st), _p(sol), *map(_p, dirs), _p(alpha), MU, KAPPA))
    S.check(S.L.iem_barrier_error(S.b, *map(_p, st), _p(r), _p(c), MU, _p(out)))


@pytest.mark.parametrize("name", sorted(LADDER))
def test_a_ladder_in_one_graph(name, built):
    """begin, four rungs of (trial, obj, cons, merit, accept), update and error captured once and replayed: bitwise the eager
    sequence, and the restatement driven by the device's f and sums; the first rung is rejected and a later one accepts"""
    import torch
    with layer(name) as S:
        P, B = S.P, S.B
        sol_h, dirs_h, alpha_h = newton_direction(P, LADDER[name])
        st = tuple(nan(k) for k in S.sizes)
        one = lambda: torch.full((1,), NAN, dtype=torch.float64, device="cuda")
        bufs = (dev(P["om"].grad(P["state"][0])), dev(sol_h), tuple(dev(d) for d in dirs_h), one(), nan(8), nan(2), nan(S.nvar), nan(S.ncon),
                [one() for _ in range(RUNGS)], [nan(S.ncon) for _ in range(RUNGS)], [nan(2) for _ in range(RUNGS)], dev(P["r"]), dev(P["c"]), nan(8))
        alpha = bufs[5]

        def load():
            for t, a in zip(st, P["state"]):
                t[:len(a)] = torch.from_numpy(a)
            alpha[:2] = torch.from_numpy(alpha_h)
            for t in [bufs[6], bufs[7], bufs[13]] + bufs[8] + bufs[9] + bufs[10]:
                t.fill_(NAN)
        load()
        S.gm.obj_device(st[0][:S.nvar], out=bufs[3])
        S.gm._sync_stream()
        S.check(S.L.iem_barrier_error(S.b, *map(_p, st), _p(bufs[11]), _p(bufs[12]), MU, _p(bufs[4])))
        f0, err_h = float(bufs[3][0]), host(bufs[4], 8)
        q = S.search()
        results = lambda: ([t.clone() for t in st] + [alpha.clone(), bufs[13].clone(), bufs[6].clone(), bufs[7].clone()] + [t.clone() for t in bufs[8] + bufs[10]],
                           q.block(), q.filter())
        load()
        _ladder(S, q, st, bufs)
        eager = results()
        # the restatement, driven by the device's f and sums of every rung
        begun = sref.begin(sref.block(status=sref.UNUSABLE), float(eager[1][sref.SLOPE]), f0, err_h, alpha_h, MU, SIGMA)
        ctl, filt, a0, statuses = begun, np.zeros((q.cap, 2)), None, []
        for k in range(RUNGS):
            ft, m = float(eager[0][11 + k][0]), host(eager[0][11 + RUNGS + k], 2)
            ctl, filt, a0 = sref.accept(ctl, filt, ft, m, MU, SIGMA, q.opts)
            statuses.append(sref.word(ctl, sref.STATUS))
        print(name, "statuses", statuses, "trials", sref.word(ctl, sref.TRIALS), "alpha", a0, "of", alpha_h[0], "phi0", ctl[sref.PHI0], "phi_t", ctl[sref.PHI_T],
              "theta0", ctl[sref.THETA0], "theta_t", ctl[sref.THETA_T])
        assert statuses[0] == sref.SEARCHING and statuses[-1] in (sref.F_TYPE, sref.H_TYPE) and sref.word(ctl, sref.TRIALS) >= 1
        assert same_bits(eager[1], ctl) and same_bits(eager[2], filt)
        assert same_bits(host(eager[0][7], 2), [a0, alpha_h[1]]) and a0 == alpha_h[0] * 0.5 ** sref.word(ctl, sref.TRIALS)
        new = bref.update(B, P["state"], sol_h, dirs_h, np.array([a0, alpha_h[1]]))
        for got, want, k, what in zip(eager[0][:7], new, S.sizes, bref_names()):
            assert same_bits(host(got, k), want), what
        assert not same_bits(new[0], P["state"][0])
        # the trial point the last rungs recomputed is the accepted one
        assert same_bits(host(eager[0][9], S.nvar), P["state"][0] + a0 * sol_h[:S.nvar])
        # captured once, replayed twice
        S.check(S.L.iem_search_reset(q.s))
        load()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            _ladder(S, q, st, bufs)
        S.gm._sync_stream()
        for _ in range(2):
            S.check(S.L.iem_search_reset(q.s))
            load()
            g.replay()
            torch.cuda.synchronize()
            again = results()
            for a, b in zip(again[0], eager[0]):
                assert torch.equal(a.view(torch.int64), b.view(torch.int64))
            assert same_bits(again[1], eager[1]) and same_bits(again[2], eager[2])
        # a ladder that never accepts: every state bit stays
        sol4, dirs4, _ = newton_direction(P, 4.0)
        bufs4 = (bufs[0], dev(sol4), tuple(dev(d) for d in dirs4)) + bufs[3:]
        q2 = S.search(max_trials=2)
        load()
        _ladder(S, q2, st, bufs4)
        torch.cuda.synchronize()
        blk = q2.block()
        print(name, "max_trials = 2:", "status", sref.word(blk, sref.STATUS), "trials", sref.word(blk, sref.TRIALS), "phi_t", blk[sref.PHI_T], "theta_t", blk[sref.THETA_T])
        assert sref.word(blk, sref.STATUS) == sref.FAILED and sref.word(blk, sref.TRIALS) == 2 and same_bits(blk[:1], [0.0])
        assert same_bits(host(alpha, 2), [0.0, alpha_h[1]])
        for got, want, k, what in zip(st, P["state"], S.sizes, bref_names()):
            assert same_bits(host(got, k), want), what


def bref_names():
    return ("x", "s", "y", "zL", "zU", "vL", "vU")


def test_refusals_and_the_python_layer(built):
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.barrier import BarrierLayer, FilterSearch
    with layer("opf_7") as S:
        P, L = S.P, S.L
        err = lambda: L.iem_last_error().decode()
        g_h, sol_h, ds_h, f_h, alpha_h = inputs(S)
        st = tuple(dev(a) for a in P["state"])
        g, sol, ds, obj, alpha = dev(g_h), dev(sol_h), dev(ds_h), dev([f_h]), dev(alpha_h)
        e8 = device_error(S, st, dev(P["r"]), dev(P["c"]))
        q = S.search()
        q.begin(st[0], st[1], g, sol, ds, obj, e8, alpha)
        before = q.block()
        xt, s_t, m2 = nan(S.nvar), nan(S.ncon), dev([1.0, 2.0])
        args = [_p(t) for t in (st[0], st[1], g, sol, ds, obj, e8, alpha)]
        for k in range(8):
            a = list(args); a[k] = None
            assert L.iem_search_begin(q.s, *a, MU, 1.0) == -4 and "null" in err(), k
        assert L.iem_search_begin(q.s, *args, -1.0, 1.0) == -4 and "mu" in err()
        targs = [_p(t) for t in (st[0], st[1], sol, ds, xt, s_t)]
        for k in range(6):
            a = list(targs); a[k] = None
            assert L.iem_search_trial(q.s, *a) == -4 and "null" in err(), k
        assert L.iem_search_accept(q.s, None, _p(m2), MU, 1.0, _p(alpha)) == -4 and "null" in err()
        assert L.iem_search_accept(q.s, _p(obj), None, MU, 1.0, _p(alpha)) == -4 and "null" in err()
        assert L.iem_search_accept(q.s, _p(obj), _p(m2), MU, 1.0, None) == -4 and "null" in err()
        assert L.iem_search_accept(q.s, _p(obj), _p(m2), -1.0, 1.0, _p(alpha)) == -4 and "mu" in err()
        out = C.c_void_p()
        for bad, word in ((dict(gamma_theta=0.0), "gamma"), (dict(gamma_phi=1.0), "gamma"), (dict(eta_phi=-1.0), "gamma"), (dict(s_theta=1.0), "s_theta"),
                          (dict(s_phi=0.5), "s_phi"), (dict(max_trials=0), "max_trials"), (dict(filter_capacity=0), "filter_capacity"),
                          (dict(filter_capacity=1025), "filter_capacity"), (dict(delta=0.0), "delta"), (dict(alpha_floor=-1.0), "alpha_floor")):
            o = iemlib.SearchOpts.defaults(**bad)
            assert L.iem_search_create(S.b, C.byref(o), C.byref(out)) == -4 and word in err(), bad
        o = iemlib.SearchOpts.defaults(); o.struct_size = 4
        assert L.iem_search_create(S.b, C.byref(o), C.byref(out)) == -4 and "struct_size" in err()
        short = iemlib.SearchState(); short.struct_size = 0
        assert L.iem_search_state(q.s, C.byref(short)) == -4 and "struct_size" in err()
        assert same_bits(q.block(), before) and np.isnan(host(xt, S.nvar)).all()      # a refused call does no device work
        # NULL options are Ipopt's defaults; a short state struct receives its head only
        raw = C.c_void_p()
        S.check(L.iem_search_create(S.b, None, C.byref(raw)))
        S.check(L.iem_search_destroy(raw))
        v = iemlib.SearchState(); v.struct_size = 24; v.phi0 = -5.0
        S.check(L.iem_search_state(q.s, C.byref(v)))
        assert v.alpha == 0.75 and v.alpha_max == 0.75 and v.phi0 == -5.0 and v.struct_size == 24
        # FilterSearch against the raw calls, bitwise
        with BarrierLayer(S.gm, relax=bref.RELAX) as bar, FilterSearch(bar, max_trials=7) as fs:
            assert fs.opts["max_trials"] == 7 and fs.opts["gamma_theta"] == 1e-5 and fs.state()["status_name"] == "unusable"
            T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
            ts = tuple(T(a) for a in P["state"])
            tg, tsol, tds, tobj, talpha, terr = T(g_h), T(sol_h), T(ds_h), T([f_h]), T(alpha_h), e8[:8].clone()
            fs.begin(ts, tg, tsol, tds, tobj, terr, talpha, MU)
            d = fs.state()
            names = ("alpha", "alpha_max", "phi0", "theta0", "slope", "theta_min", "theta_max", "phi_trial", "theta_trial")
            assert same_bits([d[k] for k in names], before[:9]) and (d["status"], d["trials"], d["filter_count"], d["flags"]) == (0, 0, 0, 1)
            txt, tst = fs.trial(ts, tsol, tds, st=torch.full((S.ncon,), NAN, dtype=torch.float64, device="cuda"))
            q.trial(st[0], st[1], sol, ds, xt, s_t)
            assert same_bits(txt.cpu().numpy(), host(xt, S.nvar)) and same_bits(tst.cpu().numpy(), host(s_t, S.ncon))
            tm = T([1e9, 0.0])      # theta_t above theta_max: rejected
            assert fs.accept(tobj, tm, MU, talpha) is talpha
            q.accept(obj, dev([1e9, 0.0]), alpha)
            d = fs.state()
            blk = q.block()
            assert same_bits([d[k] for k in names], blk[:9]) and d["status_name"] == "searching" and d["trials"] == 1 and d["alpha"] == 0.375
            assert same_bits(talpha.cpu().numpy(), host(alpha, 2)) and same_bits(talpha.cpu().numpy(), [0.0, 0.5])
            fs.reset()
            assert fs.state()["flags"] == 0
            ctl_ptr, flt_ptr = fs.device()
            assert ctl_ptr and flt_ptr
            with pytest.raises(ValueError):
                fs.begin(ts, tg[:-1], tsol, tds, tobj, terr, talpha, MU)
            with pytest.raises(iemlib.IemError, match="mu"):
                fs.accept(tobj, tm, -1.0, talpha)
            with pytest.raises(TypeError):
                FilterSearch(bar, gamma=1.0)
            with pytest.raises(iemlib.IemError, match="s_theta"):
                FilterSearch(bar, s_theta=0.5)
        with pytest.raises(iemlib.IemError, match="closed"):
            fs.reset()


@pytest.mark.parametrize("name,want", [("rosenbrock", 306.4999755050365), ("ode_5x5", -12.784599900757165)])
def test_the_pieces_make_an_algorithm(name, want, built):
    """tests/search_loop.py — BarrierLayer + KKTObject + FilterSearch, the host keeping only the mu rule and the delta_w retry — reaches
    Ipopt's error 1e-8 at the known optimum (the constants and the tolerance of tests/test_gpu_solve.py) and no search ever fails.
    Iterations (printed, not asserted; DESIGN.md 7 f4s has them)."""
    import cases
    import search_loop
    from infiniteexamodels.jl_amd import transcribe
    from infiniteexamodels.jl_amd.model import ExaModel
    core = transcribe.exa_core(cases.rosenbrock()[0]) if name == "rosenbrock" else cases.build_core(name)
    gm = ExaModel(core, device=0)
    try:
        res = search_loop.solve(gm, tol=1e-8)
        print(name, "iterations", res["iterations"], "objective", repr(res["objective"]), "error", res["error"], "mu", res["mu"], "searches", res["statuses"],
              "rungs", res["rungs_run"], "rejected trials", res["trials"])
        assert res["failed"] == 0 and set(res["statuses"]) <= {"accepted_f", "accepted_h"}, res["statuses"]
        assert res["error"] <= 1e-8 and abs(res["objective"] - want) <= 1e-6
    finally:
        gm.close()
