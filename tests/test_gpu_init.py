"""The starting point (iem_init_*, csrc/iem_init_device.h) on the MI355X.

BITWISE against tests/init_reference.py: the three outputs of iem_init_ls_terms, y and the block behind iem_init_ls_apply, the seven
state vectors behind iem_init_warm — into NaN-poisoned buffers with untouched padding, NaN planted wherever nothing may be read;
iem_init_warm with the constants of iem_barrier_start against iem_barrier_start on the device; the norm's extreme at the first and
last row and at the seam positions of the later trips; every branch of iem_init_ls_apply and iem_init_mu with the block, the
counters and a repeat, the iem_mu block against iem_mu_reset on a second object; two captured graphs replayed at two states;
tests/init_loop.py cold with and without the estimate and warm against cold; the refusals.

Shapes: those of tests/test_gpu_mu.py, whose helpers this file shares — opf_7 (two workgroups, bounds on both sides), quadrotor_100
(nz = 0), `maratos` (every row an equality) and the two big shapes of barrier_reference.big_point on 4096 workgroups:
quadrotor(27 000) (nvar + ncon > 2²⁰: a second trip, rows only) and quadrotor(60 000) (three trips, across the nvar seam)."""
import ctypes as C

import numpy as np
import pytest

import barrier_reference as bref
import init_reference as iref
import mu_reference as mref
import test_gpu_mu as tm

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")
PAD = 5
DC = 1e-8
T, H, same_bits, peek, poke = tm.T, tm.H, tm.same_bits, tm.peek, tm.poke
WARM = dict(warm_push=bref.PUSH, warm_frac=bref.FRAC, warm_z_push=0.1, warm_z_max=10.0, warm_y_max=1.0)      # every clamp bites on the shared states


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


def ls_terms(S, init, st, r):
    outs = [padded(np.full(k, NAN)) for k in (S.nvar, S.ncon, S.n)]
    init.ls_terms(st, r, out=tuple(v for _, v in outs))
    assert all(untouched(b, k) for (b, _), k in zip(outs, (S.nvar, S.ncon, S.n))), "padding touched"
    return tuple(H(v) for _, v in outs)


def ls_apply(S, init, sol_h, y_h):
    buf, y = padded(y_h)
    init.ls_apply(T(sol_h), y)
    assert untouched(buf, S.ncon), "padding touched"
    return H(y)


def warm_state(P, seed=5):
    """P's state moved so that the projection has work on every side: a third of x and s far outside, multipliers below the push,
    above the cap and NaN at present bounds, y beyond the clip on either side and NaN"""
    B = P["B"]
    rng = np.random.default_rng(seed)
    x, s, y, zL, zU, vL, vU = poisoned(B, P["state"])
    n, m = len(x), len(y)
    x = x + np.where(rng.random(n) < 0.3, 20.0 * rng.standard_normal(n), 0.0)
    s = s + np.where(rng.random(m) < 0.3, 20.0 * rng.standard_normal(m), 0.0)
    y = np.where(rng.random(m) < 0.1, NAN, 3.0 * y)
    for z, on in ((zL, B["hasL"]), (zU, B["hasU"]), (vL, B["gL"]), (vU, B["gU"])):
        idx = np.flatnonzero(on)
        if len(idx):
            z[idx[::7]] = NAN
            z[idx[3::7]] = -1.0
    x[~(B["hasL"] | B["hasU"])] = NAN      # never read: no bound
    return x, s, y, zL, zU, vL, vU


# ---- 1. bitwise ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tm.SHAPES)
def test_bitwise(name, built):
    from infiniteexamodels.jl_amd.barrier import StartingPoint
    P = tm.point(name)
    with tm.objects(P) as S, StartingPoint(S.bar) as init, StartingPoint(S.bar, **WARM) as winit:
        B = S.B
        if name in tm.BIG:
            tm.big_facts(name, S)
        # ls_terms: x and s are never read; y on equality rows is never read
        st_h = list(poisoned(B, P["state"]))
        st_h[0] = np.full(S.nvar, NAN); st_h[1] = np.full(S.ncon, NAN)
        st_h[2] = np.where(B["eq"], NAN, st_h[2])
        st = tuple(T(a) for a in st_h)
        sigma, dcon, rhs = ls_terms(S, init, st, S.r)
        want = iref.ls_terms(B, st_h, P["r"])
        print(name, "workgroups", S.bar.info["workgroups"], "nz", S.counts[1], "inequality rows", S.bar.info["n_ineq"])
        for g, w, nm in zip((sigma, dcon, rhs), want, ("sigma", "dcon", "rhs")):
            assert same_bits(g, w) and np.isfinite(g).all(), nm
        # ls_apply: sol's x part is never read; accepted, then rejected either way
        rng = np.random.default_rng(11)
        y_h = P["state"][2]
        sol_h = np.concatenate([np.full(S.nvar, NAN), 0.1 * rng.standard_normal(S.ncon)])
        blk = iref.fresh_block()
        for o, obj in ((iref.options(), init),):
            got = ls_apply(S, obj, sol_h, y_h)
            blk, want_y = iref.ls_apply(blk, y_h, sol_h, S.nvar, o)
            assert same_bits(got, want_y) and same_bits(peek(obj.device()), blk), (peek(obj.device()), blk)
            assert iref.ints(blk)[iref.ACCEPTED] == 1
        for over in (dict(y_max=1e-3), dict(y_max=1e-3, on_reject=1)):
            with StartingPoint(S.bar, **over) as tight:
                got = ls_apply(S, tight, sol_h, y_h)
                b1, want_y = iref.ls_apply(iref.fresh_block(), y_h, sol_h, S.nvar, iref.options(**over))
                assert same_bits(got, want_y) and same_bits(peek(tight.device()), b1)
                assert iref.ints(b1)[iref.ACCEPTED] == (0 if S.ncon else 1)
        # warm, every clamp biting
        w_h = warm_state(P)
        bufs = [padded(a) for a in w_h]
        winit.warm(tuple(v for _, v in bufs))
        assert all(untouched(b, len(a)) for (b, _), a in zip(bufs, w_h)), "padding touched"
        want = iref.warm(B, w_h, iref.options(**WARM))
        got = [H(v) for _, v in bufs]
        moved = [int((g.view(np.int64) != a.view(np.int64)).sum()) for g, a in zip(got, w_h)]
        print(name, "entries the projection moved (x, s, y, zL, zU, vL, vU)", moved)
        for g, w, nm in zip(got, want, ("x", "s", "y", "zL", "zU", "vL", "vU")):
            assert same_bits(g, w), nm
        assert np.isnan(got[1][B["eq"]]).all() and np.isnan(got[5][B["eq"]]).all() and np.isnan(got[6][B["eq"]]).all()      # equality rows: untouched
        assert not np.isnan(got[2]).any() and all(np.isfinite(got[k]).all() for k in (3, 4)) and moved[2] > 0
        if S.counts[1]:
            assert moved[0] > 0 and moved[3] + moved[4] + moved[5] + moved[6] > 0
        assert same_bits(peek(winit.device()), iref.fresh_block())      # warm writes no word of the block


# ---- 2. warm against iem_barrier_start ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tm.SHAPES)
def test_warm_is_barrier_start_on_the_primal_side(name, built):
    """with (bound_push, bound_frac) and s preloaded with c: x and the inequality rows of s carry the bits of iem_barrier_start"""
    import torch
    from infiniteexamodels.jl_amd.barrier import StartingPoint
    P = tm.point(name)
    with tm.objects(P) as S, StartingPoint(S.bar, warm_push=bref.PUSH, warm_frac=bref.FRAC) as init:
        B = S.B
        rng = np.random.default_rng(2)
        x_h = P["state"][0] + np.where(rng.random(S.nvar) < 0.5, 20.0 * rng.standard_normal(S.nvar), 0.0)
        c_h = P["c"] + np.where(rng.random(S.ncon) < 0.5, 20.0 * rng.standard_normal(S.ncon), 0.0)
        nanv = lambda k: torch.full((k,), NAN, dtype=torch.float64, device="cuda")
        xs = T(x_h)
        started = S.bar.start(xs, T(c_h), bound_push=bref.PUSH, bound_frac=bref.FRAC, out=(nanv(S.ncon), nanv(S.nvar), nanv(S.nvar), nanv(S.ncon), nanv(S.ncon)))
        st = poisoned(B, P["state"])
        warm = init.warm((T(x_h), T(np.where(B["eq"], NAN, c_h)), T(st[2]), *(T(a) for a in st[3:])))
        ine = ~B["eq"]
        assert same_bits(H(warm[0]), H(started[0])) and same_bits(H(warm[1])[ine], H(started[1])[ine])
        assert not same_bits(H(warm[0]), x_h) or S.counts[1] == 0


# ---- 3. the norm's extreme ----------------------------------------------------------------------------------------------------------------
def row_positions(S):
    """``[(label, row)]``: the first and the last row and every seam position that is a row"""
    pos = {"first row": S.nvar, "last row": S.n - 1}
    if S.bar.info["workgroups"] * 256 < S.n:
        pos.update({k: i for k, i in bref.seam_positions(S.nvar, S.n, S.bar.info["workgroups"]).items() if i >= S.nvar})
    out, seen = [], set()
    for label, i in pos.items():
        if i not in seen:
            seen.add(i)
            out.append((label, i - S.nvar))
    return out


@pytest.mark.parametrize("name", ["opf_7"] + list(tm.BIG))
def test_the_norm_at_the_seams(name, built):
    """ynorm with its deciding entry planted at the first row, the last row and the seam positions of the later trips in turn: word 0
    carries the bits numpy gives for the planted entry, which beats the rest; a NaN planted there rejects"""
    from infiniteexamodels.jl_amd.barrier import StartingPoint
    P = tm.point(name)
    with tm.objects(P) as S, StartingPoint(S.bar, y_max=1e300) as init:
        if name in tm.BIG:
            tm.big_facts(name, S)
        rng = np.random.default_rng(13)
        y_h = P["state"][2]
        d_h = 0.1 * rng.standard_normal(S.ncon)
        sol = T(np.concatenate([np.full(S.nvar, NAN), d_h]))
        base = float(np.abs(y_h + d_h).max())
        buf, y = padded(y_h)
        n_a = n_r = 0
        for label, j in row_positions(S):
            for value in (-1e12, NAN):
                old = float(sol[S.nvar + j])
                sol[S.nvar + j] = value
                y.copy_(T(y_h))
                init.ls_apply(sol, y)
                sol[S.nvar + j] = old
                blk = peek(init.device())
                one = np.abs(np.float64(y_h[j]) + np.float64(value))
                print(f"{name} {value} planted at {label} (row {j}): ynorm {blk[0]!r}, the rest {base!r}")
                assert untouched(buf, S.ncon)
                if value == value:
                    n_a += 1
                    assert one > base and same_bits(blk[0], one) and iref.ints(blk)[iref.ACCEPTED] == 1
                    want = y_h + d_h
                    want[j] = np.float64(y_h[j]) + np.float64(value)
                    assert same_bits(H(y), want)
                else:
                    n_r += 1
                    assert np.isnan(blk[0]) and iref.ints(blk)[iref.ACCEPTED] == 0 and same_bits(H(y), np.zeros(S.ncon))
                assert (iref.ints(blk)[iref.N_ACCEPTED], iref.ints(blk)[iref.N_REJECTED]) == (n_a, n_r)
        y.copy_(T(y_h))
        init.ls_apply(sol, y)
        assert same_bits(peek(init.device())[0], base)      # everything was put back


# ---- 4. every branch ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tm.SHAPES)
def test_branches(name, built):
    """every branch of iem_init_ls_apply and of iem_init_mu is the restatement's, with the block, the counters and a repeat; the seven
    words iem_init_mu writes into the iem_mu block are those iem_mu_reset writes on a second iem_mu object at the reference's mu0,
    and the other words stay; reset zeroes the block"""
    from infiniteexamodels.jl_amd.barrier import BarrierParameter, StartingPoint
    P = tm.point(name)
    with tm.objects(P) as S, BarrierParameter(S.bar) as other:
        nz = S.counts[1]
        rng = np.random.default_rng(17)
        y_h = P["state"][2]
        d_h = 0.1 * rng.standard_normal(S.ncon)
        top = float(np.abs(y_h + d_h).max()) if S.ncon else 0.0
        d_nan = d_h.copy()
        if S.ncon:
            d_nan[S.ncon // 2] = NAN
        x_nan = np.full(S.nvar, NAN)
        apply_cases = [("accepted", dict(), d_h), ("rejected by size", dict(y_max=top / 2), d_h), ("rejected by size, y kept", dict(y_max=top / 2, on_reject=1), d_h),
                       ("rejected by NaN", dict(), d_nan), ("rejected by NaN, y kept", dict(on_reject=1), d_nan), ("ynorm == y_max", dict(y_max=top), d_h),
                       ("the next double below", dict(y_max=float(np.nextafter(top, 0.0))), d_h)]
        decisions = []
        for label, over, d in apply_cases:
            o = iref.options(**over)
            with StartingPoint(S.bar, **over) as init:
                blk = iref.fresh_block()
                for _ in range(2):      # a repeat: the same bits, the counters go on
                    got = ls_apply(S, init, np.concatenate([x_nan, d]), y_h)
                    blk, want = iref.ls_apply(blk, y_h, np.concatenate([x_nan, d]), S.nvar, o)
                    dev = peek(init.device())
                    assert same_bits(got, want) and same_bits(dev, blk), (label, dev, blk)
                s = init.state()
                iw = iref.ints(blk)
                assert (s["accepted"], s["n_accepted"], s["n_rejected"]) == (bool(iw[1]), iw[2], iw[3]) and same_bits(s["ynorm"], blk[0]) and iw[2] + iw[3] == 2
                decisions.append((label, s["accepted"]))
                init.reset()
                assert same_bits(peek(init.device()), iref.fresh_block())
        print(name, "top", top, decisions)
        if S.ncon and top > 0.0:
            assert [a for _, a in decisions] == [True, False, False, False, False, True, False]
        # iem_init_mu
        mo = mref.options()
        assert all(S.par.opts[k] == v for k, v in mo.items())
        before = mref.fresh_block(mo)
        before[3:8] = [1.0, 2.0, 3.0, 4.0, 5.0]
        mref.ints(before)[8:12] = [1, 1, 7, 9]      # a finished solve: CONVERGED, the flag, the counters
        scale = max(nz, 1)
        mu_cases = [("average", dict(), 1e-3 * scale, 0.0), ("counted", dict(), 1e-3 * scale, 1.0), ("a NaN sum", dict(), NAN, 0.0), ("a zero sum", dict(), 0.0, 0.0),
                    ("below the floor", dict(), 1e-13 * scale, 0.0), ("above the cap", dict(), 5.0 * scale, 0.0), ("above mu_cap", dict(mu_cap=0.5), 5.0 * scale, 0.0),
                    ("under mu_cap", dict(mu_cap=0.5), 0.25 * scale, 0.0), ("mu_factor", dict(mu_factor=0.5), 1e-3 * scale, 0.0), ("an infinite sum", dict(), INF, 0.0)]
        seen = set()
        for label, over, w9, w10 in mu_cases:
            o = iref.options(**over)
            w = np.zeros(12)
            w[9], w[10] = w9, w10
            with StartingPoint(S.bar, **over) as init:
                blk = iref.fresh_block()
                for _ in range(2):
                    poke(S.blk, before)
                    init.mu(T(w), S.par)
                    blk, want = iref.mu(blk, before, w, nz, o, mo)
                    assert same_bits(peek(init.device()), blk) and same_bits(peek(S.blk), want), (label, peek(S.blk), want)
                mu0, how = float(blk[iref.MU0]), int(iref.ints(blk)[iref.HOW])
                poke(other.device(), before)
                other.reset(mu0)      # iem_mu_reset on a second object at the reference's mu0: the same seven words
                assert same_bits(peek(other.device()), peek(S.blk)), label
                s = init.state()
                assert same_bits(s["mu0"], mu0) and s["how"] == how and S.par.state()["mu"] == mu0
                seen.add(how)
                print(name, label, "mu0", mu0, "how", s["how_name"])
        assert seen == ({0, 1, 2, 3} if nz else {1})


# ---- 5. the graphs ------------------------------------------------------------------------------------------------------------------------
def test_one_graph_for_the_estimate(built):
    """ls_terms → assemble (zero Hessian) → factor_async → refined solve → ls_apply captured ONCE (device border) and replayed at two
    states: y, the solution, the terms, the inertia and the block are bitwise the uncaptured calls'.  A second graph, mu_error →
    init_mu, likewise.  Between the replays the blocks are reset by iem_init_reset and iem_mu_reset, launches on the stream."""
    import torch
    from infiniteexamodels.jl_amd.barrier import StartingPoint
    P = bref.barrier_point("opf_7")
    y_max = 2e4      # between the two estimates of this point (max |y_new| 1.2e4 and 2.5e4, printed below): one graph, both decisions
    over = dict(y_max=y_max, mu_cap=1e9)      # the cap out of the way: mu0 is the average of each state
    with tm.objects(P) as S, StartingPoint(S.bar, **over) as init:
        L = S.gm._L
        k = C.c_void_p()
        assert L.iem_kkt_create(S.gm._h, 0, C.byref(k)) == 0 and L.iem_kkt_set_border(k, 1) == 0
        try:
            p = lambda t: C.c_void_p(t.data_ptr())
            nanv = lambda *n: torch.full(n, NAN, dtype=torch.float64, device="cuda")
            st = tuple(nanv(len(a)) for a in P["state"])
            r, c, w = nanv(S.nvar), nanv(S.ncon), nanv(12)
            sigma, dcon, rhs, sol = nanv(S.nvar), nanv(S.ncon), nanv(S.n), nanv(S.n)
            inertia = torch.zeros(3, dtype=torch.int64, device="cuda")
            jv, hv = nanv(int(S.gm.meta.nnzj)), nanv(int(S.gm.meta.nnzh))
            zeros_h, zeros_y = torch.zeros_like(hv), torch.zeros(S.ncon, dtype=torch.float64, device="cuda")
            x0 = T(P["state"][0])
            S.gm.jac_hess_coord(x0, zeros_y, jv, hv, obj_weight=1.0)      # the Jacobian at the point; the Hessian values are not used
            cold = list(bref.start(S.B, P["state"][0], P["c"], tuple(np.full(S.ncon, NAN) for _ in range(3))))
            cold = (cold[0], cold[1], np.zeros(S.ncon), *cold[2:])
            states = {"cold": (cold, P["r"]), "given": (P["state"], 0.5 * P["r"])}
            iptr = init.device()

            def load(label):
                st_h, r_h = states[label]
                for t, a in zip(st, st_h):
                    t.copy_(T(a))
                r.copy_(T(r_h)); c.copy_(T(P["c"]))
                for t in (sigma, dcon, rhs, sol, w):
                    t.fill_(NAN)
                inertia.zero_()
                init.reset()      # the two blocks as created, by the objects' own launches on the stream (no host copy between the replays)
                S.par.reset()

            def estimate():
                init.ls_terms(st, r, out=(sigma, dcon, rhs))
                S.gm._sync_stream()
                assert L.iem_kkt_assemble_diag(k, p(zeros_h), p(jv), p(sigma), p(dcon), 0.0, DC) == 0
                assert L.iem_kkt_factor_async(k, p(inertia)) == 0
                assert L.iem_kkt_solve_refined_diag(k, p(x0), p(zeros_y), 0.0, p(sigma), p(dcon), 0.0, DC, 1, p(rhs), S.n, p(sol), S.n, 1, None) == 0
                init.ls_apply(sol, st[2])

            def warm_mu():
                S.par.error(st, r, c, out=w)
                init.mu(w, S.par)

            results = lambda: ([H(t) for t in (st[2], sigma, dcon, rhs, sol, w)], inertia.tolist(), peek(iptr), peek(S.blk))
            for sequence, what in ((estimate, "the estimate"), (warm_mu, "the warm mu")):
                expected = {}
                for label in ("given", "cold"):      # (the first eager sequence does the set-up)
                    load(label)
                    sequence()
                    expected[label] = results()
                    flat, inert, blk, mblk = expected[label]
                    print(what, label, "inertia", inert, "block", blk[:6].tolist(), iref.ints(blk)[:6].tolist(), "mu", mblk[0])
                if sequence is estimate:
                    for label in expected:
                        flat, inert, blk, _ = expected[label]
                        assert inert == [S.nvar, S.ncon, 0] and np.isfinite(flat[4]).all()
                        # the device's solution satisfies the dense system of the contract, built on the host from the device's own terms:
                        # 1e-9·max(1, ‖rhs‖∞, ‖sol‖∞), the tolerance of tests/test_barrier.py::test_the_algebra
                        st_h, r_h = states[label]
                        J = iref.dense_jacobian(P["om"], P["state"][0])
                        K = iref.ls_system(J, flat[1], flat[2], DC)
                        scale = max(1.0, np.abs(flat[3]).max(), np.abs(flat[4]).max())
                        worst = float(np.abs(K @ flat[4] - flat[3]).max())
                        print(what, label, "residual of the dense system", worst, "scale", scale)
                        assert worst <= 1e-9 * scale
                        assert all(same_bits(a, b) for a, b in zip(flat[1:4], iref.ls_terms(S.B, st_h, r_h)))
                        blk_ref, y_ref = iref.ls_apply(iref.fresh_block(), st_h[2], flat[4], S.nvar, iref.options(**over))
                        assert same_bits(blk, blk_ref) and same_bits(flat[0], y_ref)
                    decisions = {label: int(iref.ints(expected[label][2])[iref.ACCEPTED]) for label in expected}
                    assert decisions == {"given": 1, "cold": 0}, decisions      # the replays below cross from one decision to the other
                    assert not same_bits(expected["cold"][0][0], expected["given"][0][0])
                else:
                    for label in expected:
                        flat, _, blk, mblk = expected[label]
                        blk_ref, m_ref = iref.mu(iref.fresh_block(), mref.fresh_block(mref.options()), flat[5], S.counts[1], iref.options(**over), mref.options())
                        assert same_bits(blk, blk_ref) and same_bits(mblk, m_ref) and iref.ints(blk)[iref.HOW] == iref.FROM_AVERAGE
                    assert expected["cold"][3][0] != expected["given"][3][0]      # two barrier parameters: the replays below cross from one to the other
                load("given")
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    sequence()
                S.gm._sync_stream()
                for label in ("given", "cold", "given"):
                    load(label)
                    g.replay()
                    torch.cuda.synchronize()
                    got, want = results(), expected[label]
                    for i, (a, b) in enumerate(zip(got[0], want[0])):
                        assert same_bits(a, b), (what, label, i)
                    assert got[1] == want[1] and same_bits(got[2], want[2]) and same_bits(got[3], want[3]), (what, label)
        finally:
            torch.cuda.synchronize()
            assert L.iem_kkt_destroy(k) == 0


# ---- 6. the loops -------------------------------------------------------------------------------------------------------------------------
def _core(name):
    import cases
    from infiniteexamodels.jl_amd import transcribe
    if name == "rosenbrock":
        return transcribe.exa_core(cases.rosenbrock()[0])
    if name == "pfun":
        return transcribe.exa_core(cases.pfun()[0])
    return cases.build_core(name)


@pytest.mark.parametrize("name", ["rosenbrock", "ode_5x5", "pfun"])
def test_the_cold_loop_with_the_estimate(name, built):
    """tests/init_loop.py from iem_barrier_start alone and with the least-squares estimate behind it: both CONVERGED with error <=
    1e-8, the objectives within 1e-6 of each other, and the accepted / rejected word is the host's own evaluation of ynorm against
    y_max.  Iteration counts are printed, not asserted (DESIGN.md 7 f4i has them)."""
    import init_loop
    from infiniteexamodels.jl_amd.model import ExaModel
    gm = ExaModel(_core(name), device=0)
    try:
        plain = init_loop.solve(gm, None, tol=1e-8)
        ls = init_loop.solve(gm, "ls", tol=1e-8)
        i = ls["init"]
        print(name, "iterations without / with the estimate", plain["iterations"], ls["iterations"], "objective", repr(plain["objective"]), repr(ls["objective"]), "error",
              plain["error"], ls["error"], "ynorm", i["ynorm"], "host", i["ynorm_host"], "accepted", i["accepted"], "inertia", i["inertia"], "failed searches", plain["failed"], ls["failed"])
        for r in (plain, ls):
            assert r["status"] == mref.CONVERGED and r["error"] <= 1e-8, (r["status"], r["error"])
        assert abs(plain["objective"] - ls["objective"]) <= 1e-6
        assert same_bits(i["ynorm"], i["ynorm_host"]) and i["accepted"] == (i["ynorm_host"] <= iref.OPTS["y_max"])
        assert (i["n_accepted"], i["n_rejected"]) == (int(i["accepted"]), int(not i["accepted"]))
        assert np.abs(i["y_start"]).max() == (i["ynorm_host"] if i["accepted"] else 0.0)
    finally:
        gm.close()


def moved_bounds(gm, by=0.01):
    """the model's bounds with every finite variable and row bound moved inwards by `by`·max(1, |bound|); equality rows stay"""
    lvar, uvar, lcon, ucon = (np.array(getattr(gm.meta, k), dtype=np.float64) for k in ("lvar", "uvar", "lcon", "ucon"))
    step = lambda b: by * np.maximum(1.0, np.abs(b))
    eq = lcon == ucon
    with np.errstate(invalid="ignore"):
        return (np.where(np.isfinite(lvar), lvar + step(lvar), lvar), np.where(np.isfinite(uvar), uvar - step(uvar), uvar),
                np.where(np.isfinite(lcon) & ~eq, lcon + step(lcon), lcon), np.where(np.isfinite(ucon) & ~eq, ucon - step(ucon), ucon))


def test_the_warm_loop(built):
    """`pfun` solved to convergence, then its variable and row bounds moved by 1 % on a second BarrierLayer: the re-solve cold and the
    re-solve from the converged state through iem_init_warm, iem_mu_error and iem_init_mu both end CONVERGED within 1e-6 of each
    other, and the warm run begins at the restatement's mu0, bit for bit.  Iteration counts are printed, not asserted."""
    import init_loop
    from infiniteexamodels.jl_amd.model import ExaModel
    gm = ExaModel(_core("pfun"), device=0)
    try:
        first = init_loop.solve(gm, None, tol=1e-8)
        assert first["status"] == mref.CONVERGED and first["error"] <= 1e-8
        bounds = moved_bounds(gm)
        cold = init_loop.solve(gm, None, bounds=bounds, tol=1e-8)
        warm = init_loop.solve(gm, "warm", warm_state=first["final"], bounds=bounds, tol=1e-8)
        i = warm["init"]
        B = bref.relaxed_bounds(*bounds, 1e-8)
        mo = mref.options(tol=1e-8)
        mu0, how = iref.choose_mu(i["w"], B["counts"]["nz"], iref.options(), mo)
        print("pfun: first solve", first["iterations"], "iterations, objective", repr(first["objective"]), "; bounds moved by 1 %: cold", cold["iterations"], "warm", warm["iterations"],
              "objectives", repr(cold["objective"]), repr(warm["objective"]), "errors", cold["error"], warm["error"], "mu0", i["mu0"], i["how_name"], "avg", i["w"][9] / B["counts"]["nz"],
              "mu", ["%.3e" % v for v in warm["mus"]])
        for r in (cold, warm):
            assert r["status"] == mref.CONVERGED and r["error"] <= 1e-8, (r["status"], r["error"])
        assert abs(cold["objective"] - warm["objective"]) <= 1e-6
        assert same_bits(i["mu_start"], mu0) and same_bits(i["mu0"], mu0) and i["how"] == how
        want = iref.warm(B, first["final"], iref.options())
        for g, w_, on in zip(i["state"], want, (None, ~B["eq"], None, None, None, ~B["eq"], ~B["eq"])):
            assert same_bits(g if on is None else g[on], w_ if on is None else w_[on])
        assert abs(cold["objective"] - first["objective"]) > 1e-6      # the moved bounds bind: another optimum
    finally:
        gm.close()


# ---- 7. the refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(built):
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.barrier import BarrierLayer, BarrierParameter, StartingPoint
    P = bref.barrier_point("opf_7")
    with tm.objects(P) as S:
        L, b = S.bar._handle()
        err = lambda: L.iem_last_error().decode()
        out = C.c_void_p()
        table = [("y_max", (-1.0, NAN, INF)), ("on_reject", (2, -1)), ("warm_push", (0.0, -1.0, NAN, INF)), ("warm_frac", (0.0, 0.6, NAN)), ("warm_z_push", (0.0, -1.0, NAN)),
                 ("warm_z_max", (1e-4, NAN, INF)), ("warm_y_max", (0.0, -1.0, NAN, INF)), ("mu_factor", (0.0, -1.0, NAN, INF)), ("mu_cap", (-1.0, NAN, INF))]
        for field, bads in table:
            for bad in bads:
                o = iemlib.InitOpts.defaults(**{field: bad})
                assert L.iem_init_create(b, C.byref(o), C.byref(out)) == -4 and (field in err() or "finite" in err()), (field, bad, err())
        for field, good in (("y_max", 0.0), ("warm_frac", 0.5), ("warm_z_max", 1e-3), ("mu_cap", 0.0), ("on_reject", 1)):      # the ends of the ranges
            with StartingPoint(S.bar, **{field: good}) as ok:
                assert ok.opts[field] == good
        o = iemlib.InitOpts.defaults(); o.struct_size = 4
        assert L.iem_init_create(b, C.byref(o), C.byref(out)) == -4 and "struct_size" in err()
        assert L.iem_init_create(None, None, C.byref(out)) == -4 and L.iem_init_create(b, None, None) == -4 and "null" in err()
        raw = C.c_void_p()
        iemlib.check(L.iem_init_create(b, None, C.byref(raw)))      # NULL options: the defaults
        ptr = C.c_void_p()
        assert L.iem_init_device(raw, C.byref(ptr)) == 0 and same_bits(peek(ptr.value), iref.fresh_block())
        p = lambda t: C.c_void_p(t.data_ptr())
        nanv = lambda k: torch.full((k,), NAN, dtype=torch.float64, device="cuda")
        outs = [nanv(S.nvar), nanv(S.ncon), nanv(S.n)]
        t_args = [*map(p, S.st[2:]), p(S.r), *map(p, outs)]
        for k in range(len(t_args)):
            bad = list(t_args); bad[k] = None
            assert L.iem_init_ls_terms(raw, *bad) == -4 and "null" in err(), k
        sol, y = nanv(S.n), nanv(S.ncon)
        assert L.iem_init_ls_apply(raw, None, p(y)) == -4 and "null" in err()
        assert L.iem_init_ls_apply(raw, p(sol), None) == -4 and "null" in err()
        keep = [t.clone() for t in S.st]
        w_args = [p(t) for t in keep]
        for k in range(len(w_args)):
            bad = list(w_args); bad[k] = None
            assert L.iem_init_warm(raw, *bad) == -4 and "null" in err(), k
        w12 = T(np.zeros(12))
        par = S.par._handle()[1]
        assert L.iem_init_mu(raw, None, par) == -4 and "null" in err()
        assert L.iem_init_mu(raw, p(w12), None) == -4 and "null" in err()
        # an iem_mu of another barrier object
        with BarrierLayer(S.gm, relax=bref.RELAX, bounds=(P["lvar"], P["uvar"], P["lcon"], P["ucon"])) as bar2, BarrierParameter(bar2) as par2:
            before = peek(par2.device())
            assert L.iem_init_mu(raw, p(w12), par2._handle()[1]) == -4 and "another barrier" in err()
            assert same_bits(peek(par2.device()), before)
        # a refused call does no device work
        assert all(np.isnan(H(t)).all() for t in outs + [sol, y]) and all(same_bits(H(a), H(b_)) for a, b_ in zip(keep, S.st))
        assert same_bits(peek(ptr.value), iref.fresh_block()) and same_bits(peek(S.blk), mref.fresh_block(mref.options()))
        v = iemlib.InitState(); v.struct_size = 0
        assert L.iem_init_state(raw, C.byref(v)) == -4 and "struct_size" in err()
        assert L.iem_init_state(raw, None) == -4 and "null" in err()
        v.struct_size, v.n_accepted = 16, -5
        iemlib.check(L.iem_init_state(raw, C.byref(v)))
        assert (v.accepted, v.n_accepted, v.struct_size) == (0, -5, 16)      # a short struct receives its head only
        iemlib.check(L.iem_init_destroy(raw))
        assert L.iem_init_destroy(None) == 0
        with pytest.raises(TypeError):
            StartingPoint(S.bar, bound_push=1.0)
        with StartingPoint(S.bar, y_max=10.0) as init:
            assert init.opts["y_max"] == 10.0 and init.state() == dict(ynorm=0.0, accepted=False, n_accepted=0, n_rejected=0, mu0=0.0, how=0, how_name="average")
    with pytest.raises(iemlib.IemError, match="closed"):
        init.reset()
    # a sharded handle is refused already at iem_barrier_create: there is no barrier object to create a starting point on
    from infiniteexamodels.jl_amd.model import ExaModel
    sm = ExaModel.sharded(bref.barrier_point("quadrotor_100")["blob"], 1, 0, 2, device=0)
    try:
        with pytest.raises(iemlib.IemError, match="sharded"):
            BarrierLayer(sm)
    finally:
        sm.close()
