"""The stopping test and the kept iterate (iem_conv_*, csrc/iem_conv_device.h) on the MI355X.

BITWISE against tests/conv_reference.py: the block after every iem_conv_check and iem_conv_step, the kept buffers after iem_conv_keep,
the seven state vectors after iem_conv_restore — into NaN-poisoned buffers with untouched padding, NaN planted wherever nothing may
be read (absent bounds, equality rows of the slack side); each maximum's extreme and a NaN planted at index 0, nvar − 1, the first
row, n − 1 and both sides of entry 4096·256; every branch of both decision kernels on live objects, word 8 against word 3 of the
iem_mu block behind iem_mu_update on the same twelve words; ONE captured graph mu_error → check → keep replayed at three states and
once more while latched; tests/conv_loop.py against tests/mu_loop.py and against the reference's decisions; the refusals.

Shapes: `maratos` (nz = 0, every row an equality), opf_7 (two workgroups, bounds of every kind, inequality and equality rows),
quadrotor_100 (several workgroups), quadrotor(27 000) of barrier_reference.big_point (nvar + ncon > 2²⁰ on 4096 workgroups: the
second trip of the stride loop) and a model without rows.  The helpers are those of tests/test_gpu_mu.py."""
import ctypes as C

import numpy as np
import pytest

import barrier_reference as bref
import conv_reference as cref
import mu_reference as mref
import test_gpu_mu as tm

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")
PAD = 5
BIG = "quadrotor_27000"
SHAPES = ["maratos", "opf_7", "quadrotor_100", BIG, "no_rows"]
T, H, same_bits, peek, poke = tm.T, tm.H, tm.same_bits, tm.peek, tm.poke
up = lambda v: float(np.nextafter(v, INF))
_no_rows = []


def no_rows_point():
    """cases_scaled_phases.unconstrained (75 variables, five of them read by nothing) under bounds of every kind: no row at all"""
    if not _no_rows:
        import cases_scaled_phases
        core = cases_scaled_phases.unconstrained()
        n = int(core.nvar)
        rng = np.random.default_rng(23)
        x, kx = rng.standard_normal(n), np.arange(n) % 4
        lvar, uvar = np.where(kx & 1, x - 0.5, -INF), np.where(kx & 2, x + 0.25, INF)
        e = np.zeros(0)
        B = bref.relaxed_bounds(lvar, uvar, e, e, bref.RELAX)
        mult = lambda on: np.where(on, 10.0 ** rng.uniform(-2.0, 2.0, n), NAN)
        _no_rows.append(dict(core=core, blob=None, B=B, lvar=lvar, uvar=uvar, lcon=e, ucon=e, state=(x, e, e, mult(B["hasL"]), mult(B["hasU"]), e, e),
                             r=rng.standard_normal(n), c=e))
    return _no_rows[0]


def point(name):
    return no_rows_point() if name == "no_rows" else tm.point(name)


def padded(a):
    """a NaN-poisoned buffer holding `a` in front: ``(buffer, view)``"""
    import torch
    a = np.ascontiguousarray(a, dtype=np.float64)
    buf = torch.full((len(a) + PAD,), NAN, dtype=torch.float64, device="cuda")
    buf[:len(a)].copy_(T(a))
    return buf, buf[:len(a)]


def untouched(buf, n):
    return np.isnan(H(buf)[n:]).all()


def poisoned(B, st):
    """the state with NaN wherever no call may read: absent bounds, equality rows of the slack side"""
    x, s, y, zL, zU, vL, vU = (a.copy() for a in st)
    zL[~B["hasL"]] = NAN; zU[~B["hasU"]] = NAN; vL[~B["gL"]] = NAN; vU[~B["gU"]] = NAN
    s[B["eq"]] = NAN
    return x, s, y, zL, zU, vL, vU


def words(e=1.0, d=None, p=None, cpl=None, w10=0.0):
    """twelve words with sd = sc = 1 (w4 = w5 = 0) whose E(0) is max(d, p, cpl) where rows and bounds exist"""
    w = np.zeros(12)
    d, p, cpl = (e if v is None else v for v in (d, p, cpl))
    w[0], w[1], w[2], w[3], w[8], w[10] = d, 0.5 * d, p, cpl, 0.0, w10
    return w


def block(conv):
    return peek(conv.device(), cref.WORDS)


def held(conv):
    return tuple(H(t) for t in conv.kept())


# ---- 1. keep and restore ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPES)
def test_keep_and_restore(name, built):
    """with the word at 0 keep and restore leave every byte as it was; at 1 they copy exactly the stated entries; a worse acceptable
    point is not copied; reset zeroes the block and leaves the buffers"""
    import torch
    from infiniteexamodels.jl_amd.barrier import ConvergenceCheck
    P = point(name)
    with tm.objects(P) as S, ConvergenceCheck(S.par) as conv:
        B, mo, co = S.B, mref.options(), cref.options()
        if name == BIG:
            tm.big_facts(name, S)
        print(name, "workgroups", S.bar.info["workgroups"], "nvar", S.nvar, "ncon", S.ncon, "inequality rows", S.bar.info["n_ineq"])
        st_h = poisoned(B, P["state"])
        bufs = [padded(a) for a in st_h]
        st = tuple(v for _, v in bufs)
        zeros = cref.fresh_kept(S.nvar, S.ncon)
        nan_state = lambda: [padded(np.full(len(a), NAN)) for a in st_h]
        # the word at 0: nothing moves
        assert same_bits(block(conv), cref.fresh_block()) and all(same_bits(a, b) for a, b in zip(held(conv), zeros))
        conv.keep(st)
        assert all(same_bits(a, b) for a, b in zip(held(conv), zeros))
        outs = nan_state()
        conv.restore(tuple(v for _, v in outs))
        assert all(np.isnan(H(b)).all() for b, _ in outs)
        # an acceptable point: keep = 1
        f1 = T(np.array([-2.5]))
        ref = cref.check(cref.fresh_block(), words(1e-7), -2.5, st_h[0], S.counts, co, mo)
        conv.check(T(words(1e-7)), f1, st[0])
        assert same_bits(block(conv), ref) and cref.ints(ref)[cref.KEEP] == 1 and cref.ints(ref)[cref.STATUS] == 0
        conv.keep(st)
        want = cref.keep(ref, B, st_h, zeros)
        got = held(conv)
        for g, w_, nm in zip(got, want, ("x", "s", "y", "zL", "zU", "vL", "vU")):
            assert same_bits(g, w_), nm
        assert not any(np.isnan(g).any() for g in got[2:]) and all(untouched(b, len(a)) for (b, _), a in zip(bufs, st_h))
        assert all(same_bits(H(v), a) for (_, v), a in zip(bufs, st_h))      # keep reads only
        outs = nan_state()
        conv.restore(tuple(v for _, v in outs))
        back = cref.restore(ref, B, want, tuple(np.full(len(a), NAN) for a in st_h))
        for (b, v), w_, a, nm in zip(outs, back, st_h, ("x", "s", "y", "zL", "zU", "vL", "vU")):
            assert same_bits(H(v), w_) and same_bits(H(v), a) and untouched(b, len(a)), nm      # NaN exactly where keep reads nothing: the poisoned state again
        # a worse acceptable point: keep = 0, another state is not copied
        ref2 = cref.check(ref, words(2e-7), -3.0, st_h[0], S.counts, co, mo)
        conv.check(T(words(2e-7)), T(np.array([-3.0])), st[0])
        assert same_bits(block(conv), ref2) and cref.ints(ref2)[cref.KEEP] == 0 and cref.ints(ref2)[cref.KEPT] == 1
        other = tuple(torch.full_like(v, 7.0) for v in st)
        conv.keep(other)
        assert all(same_bits(g, w_) for g, w_ in zip(held(conv), want))
        # reset: the block zero, the buffers keep their bytes, restore touches nothing
        conv.reset()
        assert same_bits(block(conv), cref.fresh_block()) and all(same_bits(g, w_) for g, w_ in zip(held(conv), want))
        outs = nan_state()
        conv.restore(tuple(v for _, v in outs))
        assert all(np.isnan(H(b)).all() for b, _ in outs)


# ---- 2. the maxima ------------------------------------------------------------------------------------------------------------------------
def positions(S):
    """``[(label, entry)]``: index 0, nvar − 1, the first row, n − 1 and, on 4096 workgroups, both sides of entry 4096·256"""
    pos = {"entry 0": 0, "nvar - 1": S.nvar - 1}
    if S.ncon:
        pos.update({"the first row": S.nvar, "n - 1": S.n - 1})
    if S.bar.info["workgroups"] * 256 < S.n:
        pos.update({"4096*256 - 1": 4096 * 256 - 1, "4096*256": 4096 * 256})
    return list(pos.items())


@pytest.mark.parametrize("name", ["opf_7", BIG, "no_rows"])
def test_the_maxima(name, built):
    """xmax, rel and dymax with their extreme planted at every position in turn — word 14, 17, 18 carry the bits numpy gives for the
    planted entry, which beats the rest — and a NaN planted there wins"""
    from infiniteexamodels.jl_amd.barrier import ConvergenceCheck
    P = point(name)
    with tm.objects(P) as S, ConvergenceCheck(S.par, diverging_iterates_tol=INF) as conv:
        B, mo, co = S.B, mref.options(), cref.options(diverging_iterates_tol=INF)
        if name == BIG:
            tm.big_facts(name, S)
        rng = np.random.default_rng(29)
        x_h, s_h = poisoned(B, P["state"])[:2]
        sol_h = 0.1 * rng.standard_normal(S.n)
        ds_h = np.where(B["eq"], NAN, 0.1 * rng.standard_normal(S.ncon))
        x, s, sol, ds = T(x_h), T(s_h), T(sol_h), T(ds_h)
        w, f = words(1.0), T(np.array([1.0]))
        wd = T(w)
        mu = float(peek(S.blk)[0])
        ine_rows = np.concatenate([np.zeros(S.nvar, dtype=bool), ~B["eq"]])      # the rows whose slack direction rel reads
        base = (cref.xmax(x_h), *cref.stepmax(B, x_h, s_h, sol_h, ds_h))
        print(name, "xmax, rel, dymax of the state", base)
        seen = set()
        for label, i in positions(S):
            for value in (1e12, -1e12, NAN):
                # xmax: a variable
                if i < S.nvar:
                    old = x_h[i]
                    x_h[i] = value; x[i] = value
                    conv.reset(); conv.check(wd, f, x)
                    ref = cref.check(cref.fresh_block(), w, 1.0, x_h, S.counts, co, mo)
                    got = block(conv)
                    x_h[i] = old; x[i] = float(old)
                    assert same_bits(got, ref), (label, value, got, ref)
                    assert (np.isnan(got[14]) and cref.ints(got)[0] == cref.INVALID) if value != value else (same_bits(got[14], 1e12) and cref.ints(got)[0] == 0)
                    seen.add(("xmax", label))
                # rel: the variable's direction, or the slack direction of the nearest inequality row; dymax: the row itself
                k = i if i < S.nvar else bref.nearest(ine_rows, i) if ine_rows.any() else None
                if k is not None:
                    vec_h, vec = (sol_h, sol) if k < S.nvar else (ds_h, ds)
                    j = k if k < S.nvar else k - S.nvar
                    old = vec_h[j]
                    vec_h[j] = value; vec[j] = value
                    conv.reset(); conv.step((x, s), sol, ds)
                    ref = cref.step(cref.fresh_block(), B, x_h, s_h, sol_h, ds_h, mu, co, mo)
                    got = block(conv)
                    vec_h[j] = old; vec[j] = float(old)
                    den = np.float64(1.0) + np.abs(x_h[j] if k < S.nvar else s_h[j])
                    assert same_bits(got, ref), (label, value, got, ref)
                    assert np.isnan(got[17]) if value != value else (same_bits(got[17], np.float64(1e12) / den) and got[17] > base[1])
                    seen.add(("rel", label, k < S.nvar))
                if i >= S.nvar:
                    old = sol_h[i]
                    sol_h[i] = value; sol[i] = value
                    conv.reset(); conv.step((x, s), sol, ds)
                    ref = cref.step(cref.fresh_block(), B, x_h, s_h, sol_h, ds_h, mu, co, mo)
                    got = block(conv)
                    sol_h[i] = old; sol[i] = float(old)
                    assert same_bits(got, ref), (label, value, got, ref)
                    assert np.isnan(got[18]) if value != value else same_bits(got[18], 1e12)
                    seen.add(("dymax", label))
        print(name, "planted:", sorted(seen, key=str))
        conv.reset(); conv.check(wd, f, x); conv.step((x, s), sol, ds)
        got = block(conv)
        assert same_bits([got[14], got[17], got[18]], base)      # everything was put back
        assert same_bits(H(x), x_h) and same_bits(H(sol), sol_h)


# ---- 3. every branch on live objects ------------------------------------------------------------------------------------------------------
def feed(S, conv, ref, co, mo, w, f, x_h, x):
    """one iem_conv_check on the live object and on the reference: the block word for word, the state struct, word 8 against word 3
    of the iem_mu block behind iem_mu_update on the same twelve words"""
    wd = T(w)
    latched = cref.ints(ref)[cref.STATUS] != 0
    conv.check(wd, T(np.array([f])), x)
    ref = cref.check(ref, w, f, x_h, S.counts, co, mo)
    got = block(conv)
    assert same_bits(got, ref), (w, f, got, ref)
    if not latched and not np.isnan(ref[8]):      # (a latched check leaves word 8; the payload of a NaN is not part of the contract)
        S.par.update(wd)
        assert same_bits(peek(S.blk)[3], got[8]), (peek(S.blk)[3], got[8])
    return ref


@pytest.mark.parametrize("name", ["opf_7", "maratos", "no_rows"])
def test_branches(name, built):
    from infiniteexamodels.jl_amd.barrier import ConvergenceCheck
    P = point(name)
    with tm.objects(P) as S:
        mo = mref.options()
        tol = mo["tol"]
        x_h = P["state"][0]
        x = T(x_h)
        top = float(np.abs(x_h).max())
        real = tm.words(S)      # the twelve words of the live state
        a = dict(acceptable_tol=1e-3, acceptable_dual_inf_tol=2e-3, acceptable_constr_viol_tol=3e-3, acceptable_compl_inf_tol=4e-3, acceptable_iter=3)
        runs = [
            ("the live words, twice", dict(), [(real, 1.5), (real, 1.25)], None),
            ("INVALID: w10", dict(), [(words(1e-9, w10=1.0), 1.0), (words(1.0), 1.0)], cref.INVALID),
            ("INVALID: E0 NaN", dict(), [(words(1e-9, d=NAN), 1.0)], cref.INVALID),
            ("INVALID: E0 inf", dict(), [(words(1e-9, d=INF), 1.0)], cref.INVALID),
            ("INVALID: f NaN", dict(), [(words(1e-9), NAN)], cref.INVALID),
            ("INVALID: f inf", dict(), [(words(1e-9), -INF)], cref.INVALID),
            ("CONVERGED at tol", dict(acceptable_tol=1e-30), [(words(up(tol)), 1.0), (words(tol), 2.0), (words(5.0), 3.0)], cref.CONVERGED),
            ("CONVERGED at the unscaled tolerances", dict(dual_inf_tol=1e-9, constr_viol_tol=2e-9, compl_inf_tol=3e-9, acceptable_tol=1e-30),
             [(words(d=up(1e-9), p=2e-9, cpl=3e-9), 1.0), (words(d=1e-9, p=up(2e-9), cpl=3e-9), 1.0), (words(d=1e-9, p=2e-9, cpl=up(3e-9)), 1.0), (words(d=1e-9, p=2e-9, cpl=3e-9), 1.0)],
             cref.CONVERGED),
            ("inf tolerances", dict(dual_inf_tol=INF, constr_viol_tol=INF, compl_inf_tol=INF, acceptable_dual_inf_tol=INF, acceptable_constr_viol_tol=INF,
                                    acceptable_compl_inf_tol=INF, acceptable_obj_change_tol=INF, diverging_iterates_tol=INF), [(words(1e-7), 1.0), (words(tol), 1.0)], cref.CONVERGED),
            ("ACCEPTABLE: the count, the fall back, better and worse", a,
             [(words(1e-3), 1.0), (words(up(1e-3)), 1.0), (words(1e-4), 2.0), (words(2e-4), 3.0), (words(d=1e-5, p=up(3e-3), cpl=1e-5), 3.0), (words(5e-5), 4.0), (words(5e-5), 5.0),
              (words(6e-5), 6.0), (words(9.0), 7.0)], cref.ACCEPTABLE),
            ("the objective change", dict(a, acceptable_obj_change_tol=0.25, acceptable_iter=0), [(words(1e-4), 8.0), (words(1e-4), 10.0), (words(1e-4), 6.0), (words(1e-4), 6.5)], None),
            ("MAXITER", dict(max_iter=2), [(words(1.0), 1.0)] * 4, cref.MAXITER),
            ("MAXITER keeps an acceptable point", dict(max_iter=0), [(words(1e-7), 1.0)], cref.MAXITER),
            ("DIVERGING", dict(diverging_iterates_tol=float(np.nextafter(top, 0.0))), [(words(1.0), 1.0), (words(1.0), 1.0)], cref.DIVERGING),
            ("not DIVERGING at the tolerance", dict(diverging_iterates_tol=top), [(words(1.0), 1.0)], None),
        ]
        for label, over, feeds, final in runs:
            co = cref.options(**over)
            with ConvergenceCheck(S.par, **over) as conv:
                ref = cref.fresh_block()
                trail = []
                for w, f in feeds:
                    ref = feed(S, conv, ref, co, mo, w, f, x_h, x)
                    trail.append((int(cref.ints(ref)[0]), int(cref.ints(ref)[2]), int(cref.ints(ref)[3])))
                s = conv.state()
                iw = cref.ints(ref)
                assert (s["status"], s["checks"], s["acceptable_count"], s["keep"], s["kept"], s["kept_at"], s["flags"], s["tiny_count"]) == (iw[0], iw[1], iw[2], bool(iw[3]), bool(iw[4]), iw[5], iw[6], iw[7])
                assert same_bits([s[k] for k in ("e0", "dual_inf", "constr_viol", "compl_inf", "f", "f_prev", "xmax", "kept_e0", "kept_f", "rel", "dymax")], ref[8:19])
                print(name, label, "(status, count, keep) per check", trail, "->", s["status_name"])
                assert iw[0] == (final or 0), (label, trail)
                if final:      # the latch: one more check and one step write keep = 0 and nothing else
                    latched = feed(S, conv, ref, co, mo, words(3.0), 9.0, x_h, x)
                    want = ref.copy(); cref.ints(want)[cref.KEEP] = 0
                    assert same_bits(latched, want)
                    conv.step((x, None) if S.bar.info["n_ineq"] == 0 else (x, S.st[1]), T(np.zeros(S.n)), None if S.bar.info["n_ineq"] == 0 else T(np.zeros(S.ncon)))
                    assert same_bits(block(conv), want)
                    conv.reset()
                    assert same_bits(block(conv), cref.fresh_block())
        if name == "opf_7":      # the trail of the acceptable run, as the contract reads
            assert S.counts[0] > 0 and S.counts[1] > 0


@pytest.mark.parametrize("name", ["opf_7", "maratos", "no_rows"])
def test_the_tiny_step_on_live_objects(name, built):
    """every branch of conv_step_decide with mu poked into the iem_mu block: tiny at the floor twice (TINY_STEP), a large dy, mu above
    the floor (the hint), a step that is not tiny, a NaN direction"""
    from infiniteexamodels.jl_amd.barrier import ConvergenceCheck
    P = point(name)
    with tm.objects(P) as S, ConvergenceCheck(S.par) as conv:
        B, mo, co = S.B, mref.options(), cref.options()
        floor = mo["mu_floor"]
        x_h, s_h = poisoned(B, P["state"])[:2]
        slack = S.bar.info["n_ineq"] > 0
        x, s = T(x_h), T(s_h) if slack else None
        rng = np.random.default_rng(31)
        tiny_sol, big_sol = 1e-18 * rng.standard_normal(S.n), rng.standard_normal(S.n)
        tiny_ds, big_ds = (np.where(B["eq"], NAN, 1e-18 * rng.standard_normal(S.ncon)), np.where(B["eq"], NAN, rng.standard_normal(S.ncon)))
        big_dy = tiny_sol.copy()
        big_dy[S.nvar:] = 1.0
        nan_sol = tiny_sol.copy()
        nan_sol[0] = NAN
        mu_blk = peek(S.blk)

        def go(ref, sol_h, ds_h, mu):
            mu_blk[0] = mu
            poke(S.blk, mu_blk)
            conv.step((x, s), T(sol_h), T(ds_h) if slack else None)
            ref = cref.step(ref, B, x_h, s_h, sol_h, ds_h, mu, co, mo)
            got = block(conv)
            assert same_bits(got, ref), (got, ref)
            return ref

        f = lambda blk: (int(cref.ints(blk)[0]), int(cref.ints(blk)[6]), int(cref.ints(blk)[7]))
        ref = go(cref.fresh_block(), tiny_sol, tiny_ds, up(floor))
        assert f(ref) == (0, 6, 1)
        ref = go(ref, tiny_sol, tiny_ds, up(floor))
        assert f(ref) == (0, 6, 2)      # twice tiny, mu above its floor: the hint, no stop
        ref = go(ref, big_sol, big_ds, floor)
        assert f(ref) == (0, 0, 0)
        ref = go(ref, nan_sol, tiny_ds, floor)
        assert f(ref) == (0, 0, 0) and np.isnan(ref[17])
        ref = go(ref, tiny_sol, tiny_ds, floor)
        assert f(ref) == (0, 2, 1)
        if S.ncon:
            ref = go(ref, big_dy, tiny_ds, floor)
            assert f(ref) == (0, 2, 2) and same_bits(ref[18], 1.0)      # dy is not small: no stop
        ref = go(ref, tiny_sol, tiny_ds, floor)
        assert f(ref)[0] == cref.TINY_STEP and f(ref)[1] == 2
        s_ = conv.state()
        assert s_["status_name"] == "tiny_step" and s_["tiny"] and not s_["tiny_above_floor"] and s_["tiny_count"] == f(ref)[2]
        assert same_bits(go(ref, big_sol, big_ds, 1.0), ref)      # latched: nothing is written


# ---- 4. one graph -------------------------------------------------------------------------------------------------------------------------
def test_one_graph(built):
    """iem_mu_error → iem_conv_check → iem_conv_keep captured ONCE and replayed at three states — iterating; acceptable and kept;
    converged — and once more while latched: the twelve words, the block and the kept buffers are bitwise the uncaptured calls'.
    Between the replays the state is loaded by device-to-device copies and the block is reset by iem_conv_reset, a launch on the
    stream (no host copy to the device between replays)."""
    import torch
    from infiniteexamodels.jl_amd.barrier import ConvergenceCheck
    P = bref.barrier_point("opf_7")
    cases_ = {label: (Q, st) for label, Q, st, _, _, _ in mref.branch_cases("opf_7") if label in ("far from the path", "several decreases", "converged")}
    order = [("far from the path", True, cref.ITERATING), ("several decreases", True, cref.ITERATING), ("converged", False, cref.CONVERGED), ("far from the path", False, cref.CONVERGED)]
    with tm.objects(P) as S, ConvergenceCheck(S.par) as conv:
        B, mo, co = S.B, mref.options(), cref.options()
        nanv = lambda k: torch.full((k,), NAN, dtype=torch.float64, device="cuda")
        st = tuple(nanv(len(a)) for a in P["state"])
        r, c, w, f = nanv(S.nvar), nanv(S.ncon), nanv(12), nanv(1)
        sources = {label: (tuple(T(a) for a in poisoned(B, s_h)), T(Q["r"]), T(Q["c"]), T(np.array([k + 0.5]))) for k, (label, (Q, s_h)) in enumerate(cases_.items())}

        def load(label, reset):
            src = sources[label]
            for t, a in zip(st, src[0]):
                t.copy_(a)
            r.copy_(src[1]); c.copy_(src[2]); f.copy_(src[3])
            w.fill_(NAN)
            if reset:
                conv.reset()

        def sequence():
            S.par.error(st, r, c, out=w)
            conv.check(w, f, st[0])
            conv.keep(st)

        results = lambda: (H(w), block(conv), held(conv))
        expected, ref, kept_ref = [], cref.fresh_block(), cref.fresh_kept(S.nvar, S.ncon)
        for label, reset, status in order:      # (the first eager sequence does the set-up)
            load(label, reset)
            sequence()
            expected.append(results())
            words_, blk, kept = expected[-1]
            ref = cref.check(cref.fresh_block() if reset else ref, words_, float(sources[label][3][0]), cases_[label][1][0], S.counts, co, mo)
            kept_ref = cref.keep(ref, B, poisoned(B, cases_[label][1]), kept_ref)
            print(label, "reset" if reset else "no reset", "E(0)", blk[8], "status", cref.ints(blk)[0], "keep", cref.ints(blk)[3], "kept", cref.ints(blk)[4])
            assert same_bits(blk, ref) and all(same_bits(a, b) for a, b in zip(kept, kept_ref)) and cref.ints(blk)[0] == status
        facts = [(int(cref.ints(b)[3]), int(cref.ints(b)[4])) for _, b, _ in expected]
        assert facts == [(0, 0), (1, 1), (1, 1), (0, 1)], facts      # iterating; acceptable and kept; converged and kept; latched
        assert all(same_bits(a, b) for a, b in zip(expected[3][2], expected[2][2])) and not same_bits(expected[2][2][3], expected[1][2][3])
        conv.reset()
        load(order[0][0], True)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            sequence()
        S.gm._sync_stream()
        for (label, reset, _), want in zip(order, expected):
            load(label, reset)
            g.replay()
            torch.cuda.synchronize()
            got = results()
            assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), (label, got[1], want[1])
            if cref.ints(want[1])[cref.KEPT]:      # (without a kept point the buffers hold the bytes of the eager runs above)
                assert all(same_bits(a, b) for a, b in zip(got[2], want[2])), label


# ---- 5. the loops -------------------------------------------------------------------------------------------------------------------------
def _core(name):
    import cases
    from infiniteexamodels.jl_amd import transcribe
    if name == "rosenbrock":
        return transcribe.exa_core(cases.rosenbrock()[0])
    if name == "pfun":
        return transcribe.exa_core(cases.pfun()[0])
    return cases.build_core(name)


def reads(B):
    """per state vector the entries iem_conv_keep reads"""
    ine = ~B["eq"]
    every_x, every_row = np.ones(len(B["hasL"]), dtype=bool), np.ones(len(ine), dtype=bool)
    return (every_x, ine, every_row, B["hasL"], B["hasU"], ine & B["gL"], ine & B["gU"])


def same_point(got, want, B):
    return all(same_bits(g[on], w_[on]) for g, w_, on in zip(got, want, reads(B)))


@pytest.mark.parametrize("name", ["rosenbrock", "ode_5x5", "pfun"])
def test_the_loop_with_the_defaults(name, built):
    """CONVERGED at the iteration where this run's tests/mu_loop.py converges, device and reference block for block; the kept point is
    the final state, and restore into poisoned vectors gives it back bitwise"""
    import conv_loop
    import mu_loop
    from infiniteexamodels.jl_amd.model import ExaModel
    gm = ExaModel(_core(name), device=0)
    try:
        plain = mu_loop.solve(gm, True, tol=1e-8)
        got = conv_loop.solve(gm, tol=1e-8)
        s = got["state"]
        print(name, "mu_loop iterations", plain["iterations"], "status", plain["status"], "| conv_loop checks", got["checks"], s["status_name"], "E(0)", s["e0"], "d, p, cpl",
              s["dual_inf"], s["constr_viol"], s["compl_inf"], "kept at", s["kept_at"], "acceptable in a row", s["acceptable_count"])
        assert plain["status"] == mref.CONVERGED
        assert got["blocks_agree"] and same_bits(got["block"], got["ref_block"])
        assert got["status"] == cref.CONVERGED and got["checks"] == got["iterations"] == plain["iterations"]
        assert same_bits(s["e0"], plain["error"]) and s["keep"] and s["kept"] and s["kept_at"] == got["checks"]
        B = got["B"]
        assert same_point(got["kept"], got["final"], B) and same_point(got["kept"], got["ref_kept"], B)
        want = cref.restore(got["block"], B, got["kept"], tuple(np.full(len(a), NAN) for a in got["final"]))
        assert all(same_bits(a, b) for a, b in zip(got["restored"], want)) and same_point(got["restored"], got["final"], B)
        assert all(np.isnan(a[~on]).all() for a, on in zip(got["restored"], reads(B)))      # nothing else was written
    finally:
        gm.close()


@pytest.mark.parametrize("name", ["rosenbrock", "ode_5x5", "pfun"])
def test_the_loop_stops_acceptable(name, built):
    """tol = 1e-13, acceptable_tol = 1e-6, acceptable_iter = 3: ACCEPTABLE at the check the reference names, the kept point is the
    iterate of the reference's kept check, and two more iterations past the latch change neither block nor buffers"""
    import conv_loop
    from infiniteexamodels.jl_amd.model import ExaModel
    gm = ExaModel(_core(name), device=0)
    try:
        got = conv_loop.solve(gm, tol=1e-13, past_latch=2, acceptable_tol=1e-6, acceptable_iter=3)
        s, ri = got["state"], cref.ints(got["ref_block"])
        print(name, "checks", got["checks"], s["status_name"], "E(0)", s["e0"], "kept at", s["kept_at"], "kept E(0)", s["kept_e0"], "reference: status", ri[0], "checks", ri[1],
              "kept at", ri[5], "moved past the latch", got["moved_past_latch"])
        assert got["blocks_agree"] and same_bits(got["block"], got["ref_block"])
        assert got["status"] == cref.ACCEPTABLE == ri[0] and got["checks"] == ri[1] and s["acceptable_count"] == 3
        assert s["kept"] and s["kept_at"] == ri[5] == got["ref_kept_at"] and same_point(got["kept"], got["ref_kept"], got["B"])
        assert same_point(got["restored"], got["ref_kept"], got["B"])
        want = got["block"].copy(); cref.ints(want)[cref.KEEP] = 0
        assert same_bits(got["block_past_latch"], want) and all(same_bits(a, b) for a, b in zip(got["kept_past_latch"], got["kept"]))
        if any(got["moved_past_latch"]):
            assert not same_bits(got["final_past_latch"][0], got["final"][0])      # the loop went on; only the object stood still
    finally:
        gm.close()


def test_the_loop_runs_out_of_iterations(built):
    """max_iter = 5 on Rosenbrock: MAXITER at the sixth check, kept as the reference says"""
    import conv_loop
    from infiniteexamodels.jl_amd.model import ExaModel
    gm = ExaModel(_core("rosenbrock"), device=0)
    try:
        got = conv_loop.solve(gm, tol=1e-8, max_iter=5)
        s, ri = got["state"], cref.ints(got["ref_block"])
        print("rosenbrock, max_iter 5: checks", got["checks"], s["status_name"], "E(0)", s["e0"], "kept", s["kept"], "reference kept", ri[4])
        assert got["blocks_agree"] and same_bits(got["block"], got["ref_block"])
        assert got["status"] == cref.MAXITER and got["checks"] == 5 and got["iterations"] == 5
        assert s["kept"] == bool(ri[4]) and (got["ref_kept"] is None) == (not s["kept"])
        if s["kept"]:
            assert same_point(got["kept"], got["ref_kept"], got["B"])
        else:
            assert all(np.isnan(a).all() for a in got["restored"]) and not any(a.any() for a in got["kept"])
    finally:
        gm.close()


# ---- 6. the refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(built):
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.barrier import BarrierLayer, ConvergenceCheck
    P = bref.barrier_point("opf_7")
    with tm.objects(P) as S:
        L, par = S.par._handle()
        err = lambda: L.iem_last_error().decode()
        out = C.c_void_p()
        tolerances = [k for k, v in cref.OPTS.items() if isinstance(v, float)]
        assert len(tolerances) == 11
        for field in tolerances:      # each row of the range table: <= 0 and NaN are refused, +inf and the smallest positive double pass
            for bad in (0.0, -1.0, -INF, NAN):
                o = iemlib.ConvOpts.defaults(**{field: bad})
                assert L.iem_conv_create(par, C.byref(o), C.byref(out)) == -4 and field in err(), (field, bad, err())
            for good in (INF, 5e-324):
                with ConvergenceCheck(S.par, **{field: good}) as ok:
                    assert ok.opts[field] == good
        for field in ("acceptable_iter", "max_iter"):
            o = iemlib.ConvOpts.defaults(**{field: -1})
            assert L.iem_conv_create(par, C.byref(o), C.byref(out)) == -4 and field in err()
            with ConvergenceCheck(S.par, **{field: 0}) as ok:
                assert ok.opts[field] == 0
        for size in (0, 4, C.sizeof(iemlib.ConvOpts) - 8, C.sizeof(iemlib.ConvOpts) + 8):
            o = iemlib.ConvOpts.defaults(); o.struct_size = size
            assert L.iem_conv_create(par, C.byref(o), C.byref(out)) == -4 and "struct_size" in err()
        assert L.iem_conv_create(None, None, C.byref(out)) == -4 and L.iem_conv_create(par, None, None) == -4 and "null" in err()
        raw = C.c_void_p()
        iemlib.check(L.iem_conv_create(par, None, C.byref(raw)))      # NULL options: the defaults
        ptr = C.c_void_p()
        assert L.iem_conv_device(raw, C.byref(ptr)) == 0 and same_bits(peek(ptr.value, cref.WORDS), cref.fresh_block())
        p = lambda t: C.c_void_p(t.data_ptr())
        w12, f = T(np.zeros(12)), T(np.ones(1))
        c_args = [p(w12), p(f), p(S.st[0])]
        for k in range(3):
            bad = list(c_args); bad[k] = None
            assert L.iem_conv_check(raw, *bad) == -4 and "null" in err(), k
        keep = [t.clone() for t in S.st]
        k_args = [p(t) for t in keep]
        for call in (L.iem_conv_keep, L.iem_conv_restore):
            for k in range(7):
                bad = list(k_args); bad[k] = None
                assert call(raw, *bad) == -4 and "null" in err(), k
        sol, ds = T(np.zeros(S.n)), T(np.zeros(S.ncon))
        s_args = [p(S.st[0]), p(S.st[1]), p(sol), p(ds)]
        for k in range(4):
            bad = list(s_args); bad[k] = None
            assert L.iem_conv_step(raw, *bad) == -4 and "null" in err(), k
        # a refused call does no device work
        assert same_bits(peek(ptr.value, cref.WORDS), cref.fresh_block()) and all(same_bits(H(a), H(b_)) for a, b_ in zip(keep, S.st))
        v = iemlib.ConvState(); v.struct_size = 16
        assert L.iem_conv_state(raw, C.byref(v)) == -4 and "struct_size" in err()
        assert L.iem_conv_state(raw, None) == -4 and "null" in err()
        ptrs = [C.c_void_p() for _ in range(7)]
        assert L.iem_conv_kept(raw, *[C.byref(q) for q in ptrs]) == 0 and L.iem_conv_kept(raw, *[None] * 7) == 0
        sizes = (S.nvar, S.ncon, S.ncon, S.nvar, S.nvar, S.ncon, S.ncon)
        assert [q.value - ptrs[0].value for q in ptrs] == [8 * int(sum(sizes[:k])) for k in range(7)]      # 3 nvar + 4 ncon doubles, in the order of the state
        iemlib.check(L.iem_conv_destroy(raw))
        assert L.iem_conv_destroy(None) == 0
        with pytest.raises(TypeError):
            ConvergenceCheck(S.par, tol=1e-8)
        with ConvergenceCheck(S.par, max_iter=7) as conv:
            s = conv.state()
            assert conv.opts["max_iter"] == 7 and s["status"] == 0 and s["status_name"] == "iterating" and not s["keep"] and not s["kept"] and s["e0"] == 0.0
    with pytest.raises(iemlib.IemError, match="closed"):
        conv.reset()
    # a sharded handle is refused already at iem_barrier_create: there is no parameter to create a stopping test on
    from infiniteexamodels.jl_amd.model import ExaModel
    sm = ExaModel.sharded(bref.barrier_point("quadrotor_100")["blob"], 1, 0, 2, device=0)
    try:
        with pytest.raises(iemlib.IemError, match="sharded"):
            BarrierLayer(sm)
    finally:
        sm.close()
