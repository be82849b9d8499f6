"""Mehrotra's corrector (iem_mpc_*, csrc/iem_mpc_device.h) on the MI355X.

BITWISE against tests/mpc_reference.py: both columns of iem_mpc_terms, every output of iem_mpc_step and both step lengths, into
NaN-poisoned buffers with untouched padding; NaN planted wherever nothing may be read; column 0 against iem_barrier_terms on the
device; zero affine directions against iem_barrier_terms / iem_barrier_step; bound against unbound; the extreme step-length
candidates at the seam positions of the later trips; every branch of iem_mpc_select with the own block and its counters; one
iteration captured once and replayed at two states; tests/mpc_loop.py with rule and decision on the device and on the host through
bitwise the same iterates; the refusals.

Shapes: those of tests/test_gpu_mu.py, whose helpers this file shares — opf_7 (two workgroups), quadrotor_100 (several workgroups;
nz = 0), `maratos` (every row an equality) and the two big shapes of barrier_reference.big_point on 4096 workgroups:
quadrotor(27 000) (nvar + ncon > 2²⁰: the stride loop runs a second trip, rows only) and quadrotor(60 000) (nvar > 2²⁰: three trips,
the second across the nvar seam)."""
import ctypes as C

import numpy as np
import pytest

import amu_reference as aref
import barrier_reference as bref
import mpc_reference as pref
import mu_reference as mref
import test_gpu_mu as tm

pytestmark = pytest.mark.gpu
NAN = float("nan")
PAD = 5
WRONG_MU, WRONG_TAU = 123.0, 0.5
DW, DC = 1.0, 1e-8
MU, TAU = bref.MU, bref.TAU
T, H, same_bits, peek, poke = tm.T, tm.H, tm.same_bits, tm.peek, tm.poke


def padded(n, rows=None):
    """a NaN-poisoned buffer and its first n entries (of every row): ``(buffer, view)``"""
    import torch
    buf = torch.full((n + PAD,) if rows is None else (rows, n + PAD), NAN, dtype=torch.float64, device="cuda")
    return buf, (buf[:n] if rows is None else buf[:, :n])


def untouched(buf, n):
    h = H(buf)
    return np.isnan(h[..., n:]).all()


def terms(S, mpc, sol_a, dirs_a, mu, st=None):
    buf, out = padded(S.n, rows=2)
    mpc.terms(st if st is not None else S.st, S.r, S.c, sol_a, dirs_a, mu, out=out)
    assert untouched(buf, S.n), "padding touched"
    h = H(out)
    return h[0], h[1]


def step(S, mpc, sol_a, dirs_a, sol_c, mu, tau, st=None):
    """iem_mpc_step into NaN-poisoned buffers: ``(dirs, alpha)`` on the host, the padding checked"""
    sizes = (S.ncon, S.nvar, S.nvar, S.ncon, S.ncon)
    bufs = [padded(k) for k in sizes]
    abuf, alpha = padded(2)
    mpc.step(st if st is not None else S.st, sol_a, dirs_a, sol_c, mu, tau, out=tuple(v for _, v in bufs), alpha=alpha)
    assert all(untouched(b, k) for (b, _), k in zip(bufs, sizes)) and untouched(abuf, 2), "padding touched"
    return tuple(H(v) for _, v in bufs), H(alpha)


def barrier_step(S, sol, mu, tau):
    sizes = (S.ncon, S.nvar, S.nvar, S.ncon, S.ncon)
    bufs = [padded(k) for k in sizes]
    _, alpha = padded(2)
    S.bar.step(S.st, sol, mu, tau, out=tuple(v for _, v in bufs), alpha=alpha)
    return tuple(H(v) for _, v in bufs), H(alpha)


def directions(P, seed):
    """a random affine direction (amu_reference.directions: NaN on equality rows of the slack side) and a random corrected solution"""
    sol_a, dirs_a, _ = aref.directions(P, seed)
    sol_c = 0.1 * np.random.default_rng(seed + 100).standard_normal(len(sol_a))
    return sol_a, dirs_a, sol_c


@pytest.mark.parametrize("name", tm.SHAPES)
def test_terms_and_step(name, built):
    from infiniteexamodels.jl_amd.barrier import AdaptiveBarrierParameter, MehrotraCorrector
    P = tm.point(name)
    with tm.objects(P) as S, AdaptiveBarrierParameter(S.par) as amu, MehrotraCorrector(amu) as mpc:
        B, st_h = S.B, P["state"]
        if name in tm.BIG:
            tm.big_facts(name, S)
        sol_a_h, dirs_a_h, sol_c_h = directions(P, 7)
        sol_a, dirs_a, sol_c = T(sol_a_h), tuple(T(d) for d in dirs_a_h), T(sol_c_h)
        poison = lambda: tuple(np.full(S.ncon, NAN) for _ in range(3))
        # both columns; column 0 is iem_barrier_terms on the device at the same mu
        col0, col1 = terms(S, mpc, sol_a, dirs_a, MU)
        want0, want1 = pref.terms(B, st_h, P["r"], P["c"], sol_a_h, dirs_a_h, MU)
        _, _, rhs_dev = S.bar.terms(S.st, S.r, S.c, MU)
        print(name, "workgroups", S.bar.info["workgroups"], "nz", S.counts[1], "columns differ at", int((col0 != col1).sum()), "entries")
        assert same_bits(col0, want0) and same_bits(col1, want1) and same_bits(col0, H(rhs_dev))
        assert S.counts[1] == 0 or not same_bits(col0, col1)
        # the corrected step
        dirs, alpha = step(S, mpc, sol_a, dirs_a, sol_c, MU, TAU)
        want_dirs, want_alpha = pref.step(B, st_h, sol_a_h, dirs_a_h, sol_c_h, poison(), MU, TAU)
        print(name, "alpha_c", alpha.tolist())
        for g, w, nm in zip(dirs, want_dirs, ("ds", "dzL", "dzU", "dvL", "dvU")):
            assert same_bits(g, w), nm
        assert same_bits(alpha, want_alpha), (alpha, want_alpha)
        # zero affine directions: iem_barrier_terms / iem_barrier_step, bit for bit
        zsol, zdirs = T(np.zeros(S.n)), tuple(T(np.zeros(len(d))) for d in dirs_a_h)
        z0, z1 = terms(S, mpc, zsol, zdirs, MU)
        assert same_bits(z0, H(rhs_dev)) and same_bits(z1, H(rhs_dev))
        zd, za = step(S, mpc, zsol, zdirs, sol_c, MU, TAU)
        bd, ba = barrier_step(S, sol_c, MU, TAU)
        assert all(same_bits(a, b) for a, b in zip(zd, bd)) and same_bits(za, ba)
        # NaN wherever nothing may be read or nothing read is used — absent bounds, equality rows of the slack side, dy_aff, dx_aff
        # and x without a bound, y on equality rows: the same bits
        anyx, anys = B["hasL"] | B["hasU"], B["gL"] | B["gU"]
        sol_n = sol_a_h.copy()
        sol_n[:S.nvar][~anyx] = NAN
        sol_n[S.nvar:] = NAN
        ds, dzL, dzU, dvL, dvU = (d.copy() for d in dirs_a_h)
        ds[~anys] = NAN; dzL[~B["hasL"]] = NAN; dzU[~B["hasU"]] = NAN; dvL[~B["gL"]] = NAN; dvU[~B["gU"]] = NAN
        st_n = [a.copy() for a in st_h]
        st_n[0][~anyx] = NAN; st_n[1][~anys] = NAN; st_n[2][B["eq"]] = NAN
        st_n[3][~B["hasL"]] = NAN; st_n[4][~B["hasU"]] = NAN; st_n[5][~B["gL"]] = NAN; st_n[6][~B["gU"]] = NAN
        assert not anys[B["eq"]].any()
        sol_nd, dirs_nd, st_nd = T(sol_n), tuple(T(d) for d in (ds, dzL, dzU, dvL, dvU)), tuple(T(a) for a in st_n)
        n0, n1 = terms(S, mpc, sol_nd, dirs_nd, MU, st=st_nd)
        assert same_bits(n0, col0) and same_bits(n1, col1)
        nd, na = step(S, mpc, sol_nd, dirs_nd, sol_c, MU, TAU, st=st_nd)
        assert all(same_bits(a, b) for a, b in zip(nd, dirs)) and same_bits(na, alpha)
        # bound and unbound: the same bits for the same mu, tau — and the host's arguments are ignored while bound
        blk = peek(S.blk)
        blk[0], blk[1] = MU, TAU
        poke(S.blk, blk)
        mpc.bind_mu(S.par)
        b0, b1 = terms(S, mpc, sol_a, dirs_a, WRONG_MU)
        bdirs, balpha = step(S, mpc, sol_a, dirs_a, sol_c, WRONG_MU, WRONG_TAU)
        mpc.bind_mu(None)
        assert same_bits(b0, col0) and same_bits(b1, col1) and all(same_bits(a, b) for a, b in zip(bdirs, dirs)) and same_bits(balpha, alpha)
        u0, u1 = terms(S, mpc, sol_a, dirs_a, MU)      # unbound again: the host's mu rules
        assert same_bits(u0, col0) and same_bits(u1, col1)
        if S.counts[1]:
            w0, w1 = terms(S, mpc, sol_a, dirs_a, 2.0 * MU)
            assert not same_bits(w0, col0) and not same_bits(w1, col1)


def planted(S, what):
    """``[(label, entry)]``: for every seam position the nearest entry with a lower bound of its own (tests/test_gpu_barrier.py)"""
    B = S.B
    mask = {"lower": np.concatenate([B["hasL"], B["gL"]])}[what]
    out, seen = [], set()
    for label, i in bref.seam_positions(S.nvar, S.n, S.bar.info["workgroups"]).items():
        k = bref.nearest(mask, i)
        assert mask[k]
        if k not in seen:
            seen.add(k)
            out.append((f"{label} -> {k}", k))
    return out


@pytest.mark.parametrize("name", list(tm.BIG))
def test_big_extremes_on_later_trips(name, built):
    """the two step lengths of iem_mpc_step with their deciding candidate planted at each seam position in turn: the slot carries the
    bits numpy gives for the planted entry, which beats the rest of the state; a NaN direction and a point on its bound give +0.0"""
    from infiniteexamodels.jl_amd.barrier import AdaptiveBarrierParameter, MehrotraCorrector
    P = tm.point(name)
    with tm.objects(P) as S, AdaptiveBarrierParameter(S.par) as amu, MehrotraCorrector(amu) as mpc:
        B, st_h = S.B, P["state"]
        tm.big_facts(name, S)
        sol_a_h, dirs_a_h, sol_c_h = directions(P, 21)
        sol_a, dirs_a, sol_c = T(sol_a_h), tuple(T(d) for d in dirs_a_h), T(sol_c_h)
        st = tuple(t.clone() for t in S.st)
        poison = tuple(np.full(S.ncon, NAN) for _ in range(3))
        base_alpha = pref.step(B, st_h, sol_a_h, dirs_a_h, sol_c_h, poison, MU, TAU)[1]
        assert same_bits(step(S, mpc, sol_a, dirs_a, sol_c, MU, TAU, st=st)[1], base_alpha)

        def alpha_at(i, value, x_value=None):
            """mpc_step with sol_c[i] = value (and the point's entry i = x_value): the device's two step lengths, numpy's on the cut"""
            iv, ir = (np.array([i]), np.array([], dtype=np.int64)) if i < S.nvar else (np.array([], dtype=np.int64), np.array([i - S.nvar]))
            B1, st1 = bref.cut(B, iv, ir), [a.copy() for a in bref.cut_state(st_h, iv, ir)]
            a1 = (dirs_a_h[0][ir], dirs_a_h[1][iv], dirs_a_h[2][iv], dirs_a_h[3][ir], dirs_a_h[4][ir])
            vec, j = (0, i) if i < S.nvar else (1, i - S.nvar)
            if x_value is not None:
                st1[vec][0] = x_value
                st[vec][j] = x_value
            sol_c[i] = value
            got = step(S, mpc, sol_a, dirs_a, sol_c, MU, TAU, st=st)[1]
            one = pref.step(B1, tuple(st1), sol_a_h[[i]], a1, np.array([value]), tuple(np.full(len(ir), NAN) for _ in range(3)), MU, TAU)[1]
            sol_c[i] = float(sol_c_h[i])
            if x_value is not None:
                st[vec][j] = float(st_h[vec][j])
            return got, np.minimum(base_alpha, one), one

        for slot, what in ((0, "alpha_primal"), (1, "alpha_dual")):
            for label, i in planted(S, "lower"):
                value = -1e12 if slot == 0 else 1e12      # towards a lower bound: the primal step; away from it: dz < 0, the dual step (a row's ds is dy/sigs: 1e12 beats the rest of the state on every planted row)
                got, want, one = alpha_at(i, value)
                print(f"{name} {what} planted at {label}: {got.tolist()}, the entry alone {one.tolist()}, the rest {base_alpha.tolist()}")
                assert one[slot] < base_alpha[slot] and same_bits(got, want), (what, label, got, want)
        for label, i in planted(S, "lower"):
            j = i if i < S.nvar else i - S.nvar
            bound = float((B["xl"] if i < S.nvar else B["rl"])[j])
            for case, value, x_value in (("NaN direction", NAN, None), ("on its bound", -1.0 if i < S.nvar else -1e9, bound)):
                got, want, one = alpha_at(i, value, x_value)
                print(f"{name} {case} at {label}: alpha {got.tolist()}")
                assert same_bits(got[:1], [0.0]) and same_bits(one[:1], [0.0]) and same_bits(got, want), (case, label, got, one)
        assert same_bits(step(S, mpc, sol_a, dirs_a, sol_c, MU, TAU, st=st)[1], base_alpha)      # everything was put back


@pytest.mark.parametrize("name", tm.SHAPES)
def test_select_branches(name, built):
    """every branch of the decision is the restatement's: taken, the first-order buffers are bitwise the corrected ones (sol whole,
    dzL, dzU whole, ds, dvL, dvU on inequality rows, both step lengths), refused they are untouched; the own block and its counters;
    a repeat gives the same bits; reset zeroes the block"""
    from infiniteexamodels.jl_amd.barrier import AdaptiveBarrierParameter, MehrotraCorrector
    P = tm.point(name)
    with tm.objects(P) as S, AdaptiveBarrierParameter(S.par) as amu, MehrotraCorrector(amu) as mpc:
        B = S.B
        nz = S.counts[1]
        rng = np.random.default_rng(3)
        sizes = (S.n, S.ncon, S.nvar, S.nvar, S.ncon, S.ncon)
        corr_h = tuple(rng.standard_normal(k) for k in sizes)
        first_h = tuple(rng.standard_normal(k) for k in sizes)
        corr = tuple(T(a) for a in corr_h)
        alpha_h, alpha_c_h = np.array([0.25, 0.5]), np.array([0.75, 0.875])
        ab = aref.fresh_block(aref.options())
        ab[aref.AVG] = 2.0
        poke(amu.device(), ab)
        opts = pref.options()
        scale = max(nz, 1)
        cases = [("taken", [1.5 * scale, 0.0], alpha_c_h), ("NaN product", [1.5 * scale, 1.0], alpha_c_h), ("zero step length", [1.5 * scale, 0.0], np.array([0.0, 0.5])),
                 ("zero step length", [1.5 * scale, 0.0], np.array([0.5, 0.0])), ("average", [2.5 * scale, 0.0], alpha_c_h), ("average", [NAN, 0.0], alpha_c_h),
                 ("taken", [2.0 * scale, 0.0], alpha_c_h)]
        ptr = mpc.device()
        assert same_bits(peek(ptr), pref.fresh_block())
        blk_ref = pref.fresh_block()
        seen = set()
        for want, q, ac in cases * 2:      # the second round: a repeat gives the same bits (the counters go on)
            probe_h = np.array([*q, ac[0], ac[1]])
            bufs = [padded(k) for k in sizes]
            for (_, v), a in zip(bufs, first_h):
                v.copy_(T(a))
            abuf, alpha = padded(2)
            alpha.copy_(T(alpha_h))
            mpc.select(T(probe_h), T(ac), corr[0], corr[1:], bufs[0][1], tuple(v for _, v in bufs[1:]), alpha)
            assert all(untouched(b, k) for (b, _), k in zip(bufs, sizes)) and untouched(abuf, 2), "padding touched"
            taken, predicted, reason = pref.decide(probe_h, ac, 2.0, nz, opts)
            assert reason == (want if nz else "nz = 0"), (want, reason)
            seen.add(reason)
            blk_ref, ref, alpha_ref = pref.select(B, blk_ref, probe_h, ac, ab, opts, corr_h, first_h, alpha_h)
            blk = peek(ptr)
            print(name, want, "->", reason, "block", blk[:7].tolist(), mref.ints(blk)[:3].tolist())
            assert same_bits(blk, blk_ref), (want, blk, blk_ref)
            got = [H(v) for _, v in bufs]
            for g, w, f, c, nm in zip(got, ref, first_h, corr_h, ("sol", "ds", "dzL", "dzU", "dvL", "dvU")):
                assert same_bits(g, w), (want, nm)
                if not taken:
                    assert same_bits(g, f), (want, nm)
            if taken:
                ine = ~B["eq"]
                assert same_bits(got[0], corr_h[0]) and same_bits(got[2], corr_h[2]) and same_bits(got[3], corr_h[3])
                assert all(same_bits(got[k][ine], corr_h[k][ine]) and same_bits(got[k][~ine], first_h[k][~ine]) for k in (1, 4, 5))
            assert same_bits(H(alpha), alpha_ref) and same_bits(alpha_ref, ac if taken else alpha_h)
            s = mpc.state()
            iw = mref.ints(blk)
            assert (s["taken"], s["n_taken"], s["n_refused"]) == (bool(iw[0]), iw[1], iw[2]) and same_bits([s["predicted"], s["avg"], *s["alpha_c"]], blk[3:7])
        assert seen == ({"taken", "NaN product", "zero step length", "average"} if nz else {"nz = 0"})
        assert mref.ints(blk_ref)[1] + mref.ints(blk_ref)[2] == 2 * len(cases)
        # red_fact is the object's option
        with MehrotraCorrector(amu, red_fact=0.5) as tight:
            bufs = [padded(k) for k in sizes]
            for (_, v), a in zip(bufs, first_h):
                v.copy_(T(a))
            alpha = T(alpha_h)
            probe_h = np.array([1.5 * scale, 0.0, *alpha_c_h])
            tight.select(T(probe_h), T(alpha_c_h), corr[0], corr[1:], bufs[0][1], tuple(v for _, v in bufs[1:]), alpha)
            assert same_bits(peek(tight.device()), pref.select(B, pref.fresh_block(), probe_h, alpha_c_h, ab, pref.options(red_fact=0.5), corr_h, first_h, alpha_h)[0])
            assert not tight.state()["taken"] and same_bits(H(bufs[0][1]), first_h[0])
        mpc.reset()
        assert same_bits(peek(ptr), pref.fresh_block())


def _iteration(S, amu, mpc, k, bufs):
    """error, unbind, affine terms / solve / step / probe, bind, update, mpc_terms, ONE two-column solve, barrier_step on column 0,
    mpc_step on column 1, the probe of the corrected direction, select, barrier update — on the factors the solver object holds; the
    host's mu and tau are wrong wherever an object is bound"""
    b, gm, L = S.bar, S.gm, S.gm._L
    st = bufs["state"]
    p = lambda t: C.c_void_p(t.data_ptr())

    def solve(rhs, sol, nrhs):
        gm._sync_stream()
        assert L.iem_kkt_solve_refined_diag(k, p(st[0]), p(st[2]), 1.0, p(bufs["sigma"]), p(bufs["dcon"]), DW, DC, nrhs, p(rhs), S.n, p(sol), S.n, 1, None) == 0
    S.par.error(st, bufs["r"], bufs["c"], out=bufs["w"])
    with amu.affine(b):
        b.terms(st, bufs["r"], bufs["c"], 0.0, out=(bufs["sigma"], bufs["dcon"], bufs["rhs_a"]))
        solve(bufs["rhs_a"], bufs["sol_a"], 1)
        b.step(st, bufs["sol_a"], 0.0, 1.0, out=bufs["dirs_a"], alpha=bufs["alpha_a"])
        amu.probe(st, bufs["sol_a"], bufs["dirs_a"], bufs["alpha_a"], out=bufs["q"])
    amu.update(bufs["w"], bufs["q"])
    mpc.terms(st, bufs["r"], bufs["c"], bufs["sol_a"], bufs["dirs_a"], WRONG_MU, out=bufs["rhs2"])
    solve(bufs["rhs2"], bufs["sol2"], 2)
    b.step(st, bufs["sol2"][0], WRONG_MU, WRONG_TAU, out=bufs["dirs"], alpha=bufs["alpha"])
    mpc.step(st, bufs["sol_a"], bufs["dirs_a"], bufs["sol2"][1], WRONG_MU, WRONG_TAU, out=bufs["dirs_c"], alpha=bufs["alpha_c"])
    amu.probe(st, bufs["sol2"][1], bufs["dirs_c"], bufs["alpha_c"], out=bufs["q_c"])
    mpc.select(bufs["q_c"], bufs["alpha_c"], bufs["sol2"][1], bufs["dirs_c"], bufs["sol2"][0], bufs["dirs"], bufs["alpha"])
    b.update(st, bufs["sol2"][0], bufs["dirs"], bufs["alpha"], WRONG_MU)


def test_one_graph_with_the_corrector(built):
    """ONE captured iteration (no synchronisation inside: the capture would refuse it) replayed from two states: every buffer and the
    three blocks are bitwise the eager sequence from that state, and the corrector's block is the restatement's from the device's
    words.  The factors are those of the first state with delta_w = 1 — any fixed factors serve."""
    import torch
    from infiniteexamodels.jl_amd.barrier import AdaptiveBarrierParameter, MehrotraCorrector
    name = "opf_7"
    P = bref.barrier_point(name)
    far = (P, P["state"])
    near = next((Q, st) for label, Q, st, _, _, _ in mref.branch_cases(name) if label == "several decreases")
    with tm.objects(P) as S, AdaptiveBarrierParameter(S.par) as amu, MehrotraCorrector(amu) as mpc:
        L = S.gm._L
        k = C.c_void_p()
        assert L.iem_kkt_create(S.gm._h, 0, C.byref(k)) == 0 and L.iem_kkt_set_border(k, 1) == 0
        try:
            nanv = lambda *n: torch.full(n, NAN, dtype=torch.float64, device="cuda")
            dsz = (S.ncon, S.nvar, S.nvar, S.ncon, S.ncon)
            outs = ("w", "q", "q_c", "sigma", "dcon", "rhs_a", "sol_a", "alpha_a", "rhs2", "sol2", "alpha", "alpha_c")
            groups = ("dirs_a", "dirs", "dirs_c")
            bufs = dict(state=tuple(nanv(len(a)) for a in P["state"]), r=nanv(S.nvar), c=nanv(S.ncon), w=nanv(12), q=nanv(4), q_c=nanv(4), sigma=nanv(S.nvar),
                        dcon=nanv(S.ncon), rhs_a=nanv(S.n), sol_a=nanv(S.n), alpha_a=nanv(2), rhs2=nanv(2, S.n), sol2=nanv(2, S.n), alpha=nanv(2), alpha_c=nanv(2),
                        dirs_a=tuple(nanv(n) for n in dsz), dirs=tuple(nanv(n) for n in dsz), dirs_c=tuple(nanv(n) for n in dsz))
            opts, aopts, mopts = mref.options(), aref.options(), pref.options()
            blk0, ab0, qb0 = mref.fresh_block(opts), aref.fresh_block(aopts), pref.fresh_block()
            aptr, qptr = amu.device(), mpc.device()

            def load(case):
                Q, st_h = case
                for t, a in zip(bufs["state"], st_h):
                    t.copy_(T(a))
                bufs["r"].copy_(T(Q["r"])); bufs["c"].copy_(T(Q["c"]))
                for key in outs:
                    bufs[key].fill_(NAN)
                for key in groups:
                    for t in bufs[key]:
                        t.fill_(NAN)
                poke(S.blk, blk0); poke(aptr, ab0); poke(qptr, qb0)

            def results():
                flat = [H(t) for t in bufs["state"]] + [H(bufs[key]) for key in outs] + [H(t) for key in groups for t in bufs[key]]
                return flat, peek(S.blk), peek(aptr), peek(qptr)
            # the factors: the first state's matrix, sigma and dcon from terms(mu = 0)
            load(far)
            st = bufs["state"]
            jv, hv = nanv(int(S.gm.meta.nnzj)), nanv(int(S.gm.meta.nnzh))
            S.gm.jac_hess_coord(st[0], st[2], jv, hv, obj_weight=1.0)
            S.bar.terms(st, bufs["r"], bufs["c"], 0.0, out=(bufs["sigma"], bufs["dcon"], bufs["rhs_a"]))
            S.gm._sync_stream()
            p = lambda t: C.c_void_p(t.data_ptr())
            inertia = (C.c_int64 * 3)()
            assert L.iem_kkt_assemble_diag(k, p(hv), p(jv), p(bufs["sigma"]), p(bufs["dcon"]), DW, DC) == 0 and L.iem_kkt_factor(k, inertia) == 0
            S.bar.bind_mu(S.par); mpc.bind_mu(S.par)
            expected = {}
            i_q, i_qc, i_alpha_c = 7 + outs.index("q"), 7 + outs.index("q_c"), 7 + outs.index("alpha_c")
            for label, case in (("near", near), ("far", far)):      # (the first eager sequence does the set-up)
                load(case)
                _iteration(S, amu, mpc, k, bufs)
                expected[label] = results()
                flat, blk, ab, qb = expected[label]
                q_c, alpha_c = flat[i_qc], flat[i_alpha_c]
                taken, predicted, reason = pref.decide(q_c, alpha_c, ab[aref.AVG], S.counts[1], mopts)
                print(label, "mu", blk[0], "tau", blk[1], "avg", ab[9], "q_c", q_c.tolist(), "alpha_c", alpha_c.tolist(), "decision", reason, "block", qb[:7].tolist())
                iw = mref.ints(qb)
                assert (iw[0], iw[1], iw[2]) == (int(taken), int(taken), int(not taken)) and same_bits(qb[3:7], [predicted, ab[aref.AVG], *alpha_c]) and not qb[7:].any()
                assert mref.ints(blk)[8] == mref.ITERATING and np.isfinite(flat[7 + outs.index("sol2")]).all()
                if taken:      # the first-order solution is the corrected one
                    sol2 = flat[7 + outs.index("sol2")]
                    assert same_bits(sol2[0], sol2[1]) and same_bits(flat[7 + outs.index("alpha")], alpha_c)
            assert not same_bits(expected["far"][1], expected["near"][1])
            load(far)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                _iteration(S, amu, mpc, k, bufs)
            S.gm._sync_stream()
            for label, case in (("far", far), ("near", near), ("far", far)):
                load(case)
                g.replay()
                torch.cuda.synchronize()
                got, want = results(), expected[label]
                for i, (a, b) in enumerate(zip(got[0], want[0])):
                    assert same_bits(a, b), (label, i)
                for i in range(1, 4):
                    assert same_bits(got[i], want[i]), (label, i)
            mpc.bind_mu(None); S.bar.bind_mu(None)
        finally:
            torch.cuda.synchronize()
            assert L.iem_kkt_destroy(k) == 0


def _core(name):
    import cases
    from infiniteexamodels.jl_amd import transcribe
    if name == "rosenbrock":
        return transcribe.exa_core(cases.rosenbrock()[0])
    if name == "pfun":
        return transcribe.exa_core(cases.pfun()[0])
    return cases.build_core(name)


@pytest.mark.parametrize("name,want", [("rosenbrock", 306.4999755050365), ("ode_5x5", -12.784599900757165), ("pfun", None)])
def test_the_loop_with_the_corrector(name, want, built):
    """tests/mpc_loop.py with rule and decision on the device and with the restatements on the host: bitwise the same x after every
    iteration and the same decisions, the optimum and the error of tests/test_gpu_amu.py::test_the_loop_with_the_adaptive_rule, no
    failed search.  `pfun` — the bounded linear model of tests/test_mpc.py, which KKTObject accepts — is held to the optimum of the
    same loop without the corrector, to 1e-6.  Iteration counts with and without the corrector and the taken / refused counts are
    printed, not asserted (DESIGN.md 7 f4p has them)."""
    import mpc_loop
    from infiniteexamodels.jl_amd.model import ExaModel
    gm = ExaModel(_core(name), device=0)
    try:
        plain = mpc_loop.solve(gm, True, corrector=False, tol=1e-8)
        res = {flag: mpc_loop.solve(gm, flag, tol=1e-8) for flag in (True, False)}
        print(name, "without the corrector: iterations", plain["iterations"], "objective", repr(plain["objective"]), "error", plain["error"])
        if want is None:
            assert plain["failed"] == 0 and plain["status"] == mref.CONVERGED and plain["error"] <= 1e-8
            want = plain["objective"]
        for flag, r in res.items():
            print(name, "device_rule", flag, "iterations", r["iterations"], "objective", repr(r["objective"]), "error", r["error"], "taken", r["taken"], "refused",
                  r["refused"], "searches", r["statuses"], "mu", ["%.3e" % v for v in r["mus"]])
            assert r["failed"] == 0 and set(r["statuses"]) <= {"accepted_f", "accepted_h"}, r["statuses"]
            assert r["status"] == mref.CONVERGED and r["error"] <= 1e-8 and abs(r["objective"] - want) <= 1e-6
        a, b = res[True], res[False]
        assert a["iterations"] == b["iterations"] and len(a["iterates"]) == len(b["iterates"]) == a["iterations"]
        for i, (xa, xb) in enumerate(zip(a["iterates"], b["iterates"])):
            assert same_bits(xa, xb), i
        assert same_bits(a["mus"], b["mus"]) and a["decisions"] == b["decisions"] and (a["taken"], a["refused"]) == (b["taken"], b["refused"])
    finally:
        gm.close()


def test_refusals(built):
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.barrier import AdaptiveBarrierParameter, BarrierParameter, MehrotraCorrector
    P = bref.barrier_point("opf_7")
    with tm.objects(P) as S, AdaptiveBarrierParameter(S.par) as amu:
        L, a = amu._handle()
        err = lambda: L.iem_last_error().decode()
        out = C.c_void_p()
        for bad in (0.0, -1.0, NAN, float("inf")):
            o = iemlib.MpcOpts.defaults(red_fact=bad)
            assert L.iem_mpc_create(a, C.byref(o), C.byref(out)) == -4 and "red_fact" in err(), bad
        o = iemlib.MpcOpts.defaults(); o.struct_size = 4
        assert L.iem_mpc_create(a, C.byref(o), C.byref(out)) == -4 and "struct_size" in err()
        assert L.iem_mpc_create(None, None, C.byref(out)) == -4 and L.iem_mpc_create(a, None, None) == -4 and "null" in err()
        raw = C.c_void_p()
        iemlib.check(L.iem_mpc_create(a, None, C.byref(raw)))      # NULL options: the default
        ptr = C.c_void_p()
        assert L.iem_mpc_device(raw, C.byref(ptr)) == 0 and same_bits(peek(ptr.value), pref.fresh_block())
        sol_a_h, dirs_a_h, sol_c_h = directions(P, 7)
        p = lambda t: C.c_void_p(t.data_ptr())
        import torch
        sol_a, dirs_a, sol_c = T(sol_a_h), [T(d) for d in dirs_a_h], T(sol_c_h)
        rhs2 = torch.full((2, S.n), NAN, dtype=torch.float64, device="cuda")
        outs = [torch.full((k,), NAN, dtype=torch.float64, device="cuda") for k in (S.ncon, S.nvar, S.nvar, S.ncon, S.ncon, 2)]
        first = [torch.full((k,), NAN, dtype=torch.float64, device="cuda") for k in (S.n, S.ncon, S.nvar, S.nvar, S.ncon, S.ncon, 2)]
        q4 = T(np.zeros(4))
        t_args = [*map(p, S.st), p(S.r), p(S.c), p(sol_a), *map(p, dirs_a)]
        for k in range(len(t_args)):
            b = list(t_args); b[k] = None
            assert L.iem_mpc_terms(raw, *b, MU, p(rhs2), S.n) == -4 and "null" in err(), k
        assert L.iem_mpc_terms(raw, *t_args, MU, None, S.n) == -4 and "null" in err()
        assert L.iem_mpc_terms(raw, *t_args, MU, p(rhs2), S.n - 1) == -4 and "ld" in err()
        assert L.iem_mpc_terms(raw, *t_args, -1.0, p(rhs2), S.n) == -4 and "mu" in err()
        assert L.iem_mpc_terms(raw, *t_args, NAN, p(rhs2), S.n) == -4 and "mu" in err()
        s_args = [*map(p, S.st), p(sol_a), *map(p, dirs_a), p(sol_c)]
        o_args = [*map(p, outs)]
        for k in range(len(s_args)):
            b = list(s_args); b[k] = None
            assert L.iem_mpc_step(raw, *b, MU, TAU, *o_args) == -4 and "null" in err(), k
        for k in range(len(o_args)):
            b = list(o_args); b[k] = None
            assert L.iem_mpc_step(raw, *s_args, MU, TAU, *b) == -4 and "null" in err(), k
        for mu, tau, word in ((-1.0, TAU, "mu"), (MU, 0.0, "tau"), (MU, 1.5, "tau"), (MU, NAN, "tau")):
            assert L.iem_mpc_step(raw, *s_args, mu, tau, *o_args) == -4 and word in err()
        c_args = [p(q4), p(outs[5]), p(sol_c), *map(p, outs[:5]), *map(p, first)]
        for k in range(len(c_args)):
            b = list(c_args); b[k] = None
            assert L.iem_mpc_select(raw, *b) == -4 and "null" in err(), k
        b = list(c_args); b[-1] = b[1]
        assert L.iem_mpc_select(raw, *b) == -4 and "two buffers" in err()
        # a refused call does no device work
        assert np.isnan(H(rhs2)).all() and all(np.isnan(H(t)).all() for t in outs + first) and same_bits(peek(ptr.value), pref.fresh_block())
        # bind: only the object's own iem_mu
        with BarrierParameter(S.bar) as other:
            assert L.iem_mpc_bind_mu(raw, other._handle()[1]) == -4 and "iem_mu" in err()
        assert L.iem_mpc_bind_mu(raw, S.par._handle()[1]) == 0
        assert L.iem_mpc_terms(raw, *t_args, -1.0, p(rhs2), S.n) == 0      # bound: the host's mu and its range check are ignored
        assert L.iem_mpc_bind_mu(raw, None) == 0
        v = iemlib.MpcState(); v.struct_size = 0
        assert L.iem_mpc_state(raw, C.byref(v)) == -4 and "struct_size" in err()
        assert L.iem_mpc_state(raw, None) == -4 and "null" in err()
        v.struct_size, v.n_refused = 16, -5
        iemlib.check(L.iem_mpc_state(raw, C.byref(v)))
        assert (v.taken, v.n_refused, v.struct_size) == (0, -5, 16)      # a short struct receives its head only
        iemlib.check(L.iem_mpc_destroy(raw))
        assert L.iem_mpc_destroy(None) == 0
        with pytest.raises(TypeError):
            MehrotraCorrector(amu, kappa=1.0)
        with MehrotraCorrector(amu, red_fact=0.5) as mpc:
            assert mpc.opts["red_fact"] == 0.5 and mpc.state() == dict(taken=False, n_taken=0, n_refused=0, predicted=0.0, avg=0.0, alpha_c=[0.0, 0.0])
    with pytest.raises(iemlib.IemError, match="closed"):
        mpc.reset()
