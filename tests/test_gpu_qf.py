"""The quality-function oracle (iem_qf_*, csrc/iem_qf_device.h) on the MI355X.

BITWISE against tests/qf_reference.py, whose sums have the device's order for the device's grid: the own block after iem_qf_begin,
after every iem_qf_alpha and every iem_qf_value of a full section, and after the pairs behind its end; the three blocks and a
search's control block after iem_qf_update.  Cross-checks against shipped kernels: with d1 = d0 the two slots of iem_qf_alpha are
the alphas of iem_barrier_step(mu = 0, tau = the block's); with zero directions and the slots at (1, 1) C2 is the restatement's sum
of squared complementarity products.  ONE graph — the two-column solve, both steps, begin, all pairs and the update — captured once
replays at two states; tests/qf_loop.py converges with the rule on the device and with the restatement on the host through bitwise
the same iterates.

Shapes: those of tests/test_gpu_amu.py's probe (tests/test_gpu_mu.py's) — opf_7 (two workgroups), quadrotor_100 (several workgroups:
the last-arrival path; nz = 0, the section is DONE at once), `maratos` (every row an equality) and quadrotor(27 000) with random
bounds and state (nvar + ncon > 2²⁰: the grid-stride loop runs, both ticket levels)."""
import ctypes as C

import numpy as np
import pytest

import amu_reference as aref
import barrier_reference as bref
import mu_reference as mref
import qf_reference as qref
import test_gpu_mu as tm

pytestmark = pytest.mark.gpu
NAN = float("nan")
DW, DC = 1.0, 1e-8
T, H, same_bits, peek, poke = tm.T, tm.H, tm.same_bits, tm.peek, tm.poke


def columns(P, seeds=(7, 8), mu_ref=1.0):
    """two random sol = [dx; dy] and, from them, barrier_reference.step at tau = 1 and mu = 0 / mu_ref: ``(d0, d1)`` on the host, each
    (sol, ds, dzL, dzU, dvL, dvU) — NaN on the equality rows of the slack side"""
    B, st = P["B"], P["state"]
    n, m = len(st[0]), len(st[1])
    out = []
    for seed, mu in zip(seeds, (0.0, mu_ref)):
        sol = 0.1 * np.random.default_rng(seed).standard_normal(n + m)
        dirs, _ = bref.step(B, st, sol, tuple(np.full(m, NAN) for _ in range(3)), mu, 1.0)
        out.append((sol, *dirs))
    return out


def dev(d):
    return tuple(T(a) for a in d)


@pytest.mark.parametrize("name", tm.SHAPES)
def test_begin_and_a_full_section_are_the_restatement(name, built):
    """the own block after begin, after every alpha and after every value of max_section_steps + 4 pairs, and after three pairs more
    (gated: no byte moves) — bitwise the restatement from the device's twelve words; twice from the same state: the same bits"""
    from infiniteexamodels.jl_amd.barrier import AdaptiveBarrierParameter, QualityFunction
    P = tm.point(name)
    with tm.objects(P) as S, AdaptiveBarrierParameter(S.par) as amu, QualityFunction(amu) as qf:
        B, st_h = S.B, P["state"]
        n_wg = S.bar.info["workgroups"]
        aopts, qopts = aref.options(), qref.options(aref.options())
        assert qf.opts == qopts and qf.pairs == 12
        ptr = qf.device()
        assert same_bits(peek(ptr, 32), qref.fresh_block())
        d0_h, d1_h = columns(P)
        d0, d1 = dev(d0_h), dev(d1_h)
        w = tm.words(S)
        wd = T(w)
        blk, ab = peek(S.blk), peek(amu.device())
        finals = []
        for again in range(2):
            qf.begin(S.st, S.r, S.c, wd)
            got = peek(ptr, 32)
            ref = qref.begin(B, st_h, P["r"], P["c"], w, ab, aopts, qopts, n_wg)
            print(name, "workgroups", n_wg, "nz", S.counts[1], "D2", got[qref.D2], "P2", got[qref.P2], "avg", got[qref.AVG], "lo", got[qref.LO], "hi", got[qref.HI],
                  "sigma", got[qref.SIGMA])
            assert same_bits(got, ref), (got, ref)
            evaluated = 0
            for k in range(qf.pairs + 3):
                qf.alpha(S.st, d0, d1)
                got = peek(ptr, 32)
                ref = qref.alpha(B, st_h, d0_h, d1_h, ref, blk, qopts)
                assert same_bits(got, ref), (k, "alpha", got, ref)
                running = qref.ints(ref)[qref.STATUS] == qref.SECTION
                qf.value(S.st, d0, d1)
                got = peek(ptr, 32)
                ref = qref.value(B, st_h, d0_h, d1_h, ref, qopts, n_wg)
                if running and not again:
                    print("   pair", k, "alpha", got[qref.LAST_AP], got[qref.LAST_AD], "C2", got[qref.C2], "q", got[qref.Q], "next sigma", got[qref.SIGMA],
                          "status", qref.ints(got)[qref.STATUS])
                assert same_bits(got, ref), (k, "value", got, ref)
                evaluated += int(running)
            iq = qref.ints(got)
            assert evaluated == iq[qref.EVALS] <= qf.pairs
            if S.counts[1] == 0:
                assert iq[qref.STATUS] == qref.DONE and evaluated == 0
            else:
                assert iq[qref.STATUS] in (qref.DONE, qref.UNUSABLE) and evaluated >= 2
            finals.append(got)
            s = qf.state()
            assert s["section"]["status"] == iq[qref.STATUS] and s["section"]["evaluations"] == evaluated and same_bits(s["section"]["sigma"], got[qref.BEST])
            assert same_bits([s["section"][k] for k in ("d2", "p2", "avg", "lo", "hi", "a", "b", "c", "d", "qc", "qd", "sigma", "q", "q_first")], got[7:21])
            assert same_bits(s["mu"], blk[0]) and s["mode"] == 0
        assert same_bits(finals[0], finals[1])
        assert same_bits(peek(S.blk), blk) and same_bits(peek(amu.device()), ab)      # begin, alpha and value write the own block only
        qf.reset()
        assert same_bits(peek(ptr, 32), qref.fresh_block())
        # NaN wherever nothing may be read — y, dy, absent bounds' multipliers and directions, equality rows: the same bits
        if S.counts[1]:
            def poison(d):
                sol, ds, dzL, dzU, dvL, dvU = (a.copy() for a in d)
                sol[S.nvar:] = NAN
                ds[B["eq"]] = NAN; dzL[~B["hasL"]] = NAN; dzU[~B["hasU"]] = NAN; dvL[~B["gL"]] = NAN; dvU[~B["gU"]] = NAN
                return sol, ds, dzL, dzU, dvL, dvU
            st_n = [a.copy() for a in st_h]
            st_n[3][~B["hasL"]] = NAN; st_n[4][~B["hasU"]] = NAN; st_n[5][~B["gL"]] = NAN; st_n[6][~B["gU"]] = NAN
            qf.begin(S.st, S.r, S.c, wd)
            st_y = list(st_n)
            st_y[2] = np.full(S.ncon, NAN)
            qf.section(tuple(T(a) for a in st_y), dev(poison(d0_h)), dev(poison(d1_h)))
            assert same_bits(peek(ptr, 32), finals[0])


@pytest.mark.parametrize("name", ["opf_7", "quadrotor_27000"])
def test_against_the_shipped_kernels(name, built):
    """d1 = d0: the direction is d0, so the two slots are the alphas of iem_barrier_step(mu = 0, tau = word 1 of the block) on the same
    sol (no NaN in dy) — bit for bit.  Zero directions and the slots left at (1, 1): C2 is the sum of the squared complementarity
    products in the restatement's (the device's) order, the count of NaNs zero."""
    import torch
    from infiniteexamodels.jl_amd.barrier import AdaptiveBarrierParameter, QualityFunction
    P = tm.point(name)
    with tm.objects(P) as S, AdaptiveBarrierParameter(S.par) as amu, QualityFunction(amu) as qf:
        B, st_h = S.B, P["state"]
        n_wg = S.bar.info["workgroups"]
        ptr = qf.device()
        blk = peek(S.blk)
        wd = T(tm.words(S))
        sol = T(0.1 * np.random.default_rng(11).standard_normal(S.n))
        alpha = torch.full((2,), NAN, dtype=torch.float64, device="cuda")
        dirs, _ = S.bar.step(S.st, sol, 0.0, float(blk[1]), alpha=alpha)
        d = (sol, *dirs)
        qf.begin(S.st, S.r, S.c, wd)
        seeded = peek(ptr, 32)
        assert same_bits(seeded[[qref.ALPHA_P, qref.ALPHA_D]], [1.0, 1.0])
        qf.alpha(S.st, d, d)
        got = peek(ptr, 32)
        print(name, "barrier_step", H(alpha).tolist(), "qf_alpha", got[[qref.ALPHA_P, qref.ALPHA_D]].tolist(), "tau", blk[1])
        assert same_bits(got[[qref.ALPHA_P, qref.ALPHA_D]], H(alpha)) and H(alpha)[0] > 0.0 and H(alpha)[1] > 0.0
        assert same_bits(np.delete(got, [qref.ALPHA_P, qref.ALPHA_D]), np.delete(seeded, [qref.ALPHA_P, qref.ALPHA_D]))
        # zero directions, the slots at (1, 1)
        zero = (T(np.zeros(S.n)), *(T(np.zeros(k)) for k in (S.ncon, S.nvar, S.nvar, S.ncon, S.ncon)))
        qf.begin(S.st, S.r, S.c, wd)
        qf.value(S.st, zero, zero)
        got = peek(ptr, 32)
        p = mref.products(B, st_h)
        pL, pU = qref.products(B, st_h, tuple(np.zeros(k) for k in (S.n, S.ncon, S.nvar, S.nvar, S.ncon, S.ncon)), 1.0, 1.0)
        c2 = qref.device_sum([pL * pL, pU * pU], n_wg)
        fs, bound = bref.sum_bound(p * p)
        print(name, "C2", got[qref.C2], "restated", c2, "fsum", fs, "bound", bound)
        assert same_bits(got[qref.C2], c2) and abs(got[qref.C2] - fs) <= bound
        assert same_bits(got[[qref.NANS, qref.LAST_AP, qref.LAST_AD]], [0.0, 1.0, 1.0]) and qref.ints(got)[qref.EVALS] == 1
        assert same_bits(got[qref.Q], c2 / np.float64(S.counts[1]))      # alpha = (1, 1): the residual terms vanish


@pytest.mark.parametrize("name", ["opf_7"])
def test_update_branches(name, built):
    """the three blocks and the search's control block are the restatement's on every entry of amu_reference.branch_cases with a
    finished section (unclamped, clamped at mu_min, clamped at mu_max), and with a section that is not DONE"""
    from infiniteexamodels.jl_amd.barrier import AdaptiveBarrierParameter, BarrierParameter, FilterSearch, QualityFunction
    P = tm.point(name)
    with tm.objects(P) as S, FilterSearch(S.bar) as fs:
        for case in aref.branch_cases(aref.LOQO, S.counts):
            opts, aopts, label = case["opts"], case["aopts"], case["label"]
            over = {k: v for k, v in opts.items() if v != mref.options()[k]}
            aover = {k: v for k, v in aopts.items() if v != aref.OPTS[k]}
            with BarrierParameter(S.bar, **over) as par, AdaptiveBarrierParameter(par, **aover) as amu, QualityFunction(amu) as qf:
                ptr, aptr, qptr = par.device(), amu.device(), qf.device()
                wd = T(case["w"])
                unusable = qref.done_block(0.3)
                qref.ints(unusable)[qref.STATUS] = qref.UNUSABLE
                for qb in (qref.done_block(0.3, 2.5), qref.done_block(1e-14), qref.done_block(1e6), qref.fresh_block(), unusable):
                    poke(ptr, case["blk"]); poke(aptr, case["ab"]); poke(qptr, qb)
                    ctl_ptr, flt_ptr, ctl, flt = tm.pattern_search(S, fs)
                    qf.update(wd, force_fixed=case["force_fixed"], search=fs)
                    ref, ab_ref, ctl_ref = qref.update(case["blk"], case["ab"], qb, case["w"], S.counts, opts, aopts, case["force_fixed"], ctl)
                    blk, ab = peek(ptr), peek(aptr)
                    print(name, label, "section", qref.ints(qb)[qref.STATUS], "sigma", qb[qref.BEST], "mu", blk[0], "status", mref.ints(blk)[8], "mode", mref.ints(ab)[0])
                    assert same_bits(blk, ref) and same_bits(ab, ab_ref) and same_bits(peek(qptr, 32), qb), label
                    assert same_bits(peek(ctl_ptr), ctl_ref) and same_bits(peek(flt_ptr, len(flt)), flt), label
                    s = qf.state()
                    assert same_bits([s["mu"], s["tau"], s["e0"], s["sigma"], s["mu_oracle"]], [blk[0], blk[1], blk[3], ab[aref.SIGMA], ab[aref.MU_ORACLE]])
                    assert s["status"] == mref.ints(blk)[8] and s["mode"] == mref.ints(ab)[0] and s["section"]["status"] == qref.ints(qb)[qref.STATUS]
                    if qref.ints(qb)[qref.STATUS] != qref.DONE:
                        assert s["status_name"] == "unusable"


def _iteration(S, fs, amu, qf, k, bufs):
    """error, unbind, terms at mu = 0 and mu_ref, ONE two-column solve, both steps, bind, begin, all pairs, update, terms, solve, step,
    search begin, one rung, barrier update — on the factors the solver object holds; the host's mu and tau are wrong wherever an
    object is bound"""
    b, gm, L = S.bar, S.gm, S.gm._L
    st = bufs["state"]
    p = lambda t: C.c_void_p(t.data_ptr())

    def solve(rhs, sol, nrhs):
        gm._sync_stream()
        assert L.iem_kkt_solve_refined_diag(k, p(st[0]), p(st[2]), 1.0, p(bufs["sigma"]), p(bufs["dcon"]), DW, DC, nrhs, p(rhs), S.n, p(sol), S.n, 1, None) == 0
    S.par.error(st, bufs["r"], bufs["c"], out=bufs["w"])
    with amu.affine(b, fs):
        b.terms(st, bufs["r"], bufs["c"], 0.0, out=(bufs["sigma"], bufs["dcon"], bufs["rhs2"][0]))
        b.terms(st, bufs["r"], bufs["c"], qf.opts["mu_ref"], out=(bufs["sigma"], bufs["dcon"], bufs["rhs2"][1]))
        solve(bufs["rhs2"], bufs["sol2"], 2)
        b.step(st, bufs["sol2"][0], 0.0, 1.0, out=bufs["dirs0"], alpha=bufs["alpha0"])
        b.step(st, bufs["sol2"][1], qf.opts["mu_ref"], 1.0, out=bufs["dirs1"], alpha=bufs["alpha1"])
    qf.begin(st, bufs["r"], bufs["c"], bufs["w"])
    qf.section(st, (bufs["sol2"][0], *bufs["dirs0"]), (bufs["sol2"][1], *bufs["dirs1"]))
    qf.update(bufs["w"], search=fs)
    b.terms(st, bufs["r"], bufs["c"], tm.WRONG_MU, out=(bufs["sigma"], bufs["dcon"], bufs["rhs"]))
    solve(bufs["rhs"], bufs["sol"], 1)
    b.step(st, bufs["sol"], tm.WRONG_MU, tm.WRONG_TAU, out=bufs["dirs"], alpha=bufs["alpha"])
    fs.begin(st, bufs["g"], bufs["sol"], bufs["dirs"][0], bufs["f"], bufs["w"][:8], bufs["alpha"], tm.WRONG_MU)
    fs.trial(st, bufs["sol"], bufs["dirs"][0], bufs["xt"], bufs["s_t"])
    gm.obj_device(bufs["xt"], out=bufs["ft"])
    gm.cons(bufs["xt"], bufs["ct"])
    b.merit(bufs["xt"], bufs["s_t"], bufs["ct"], out=bufs["mt"])
    fs.accept(bufs["ft"], bufs["mt"], tm.WRONG_MU, bufs["alpha"])
    b.update(st, bufs["sol"], bufs["dirs"], bufs["alpha"], tm.WRONG_MU)


def test_one_graph_with_the_section(built):
    """ONE captured iteration (no synchronisation inside: the capture would refuse it) replayed from two states: every buffer, the
    three blocks, the search's block and its filter are bitwise the eager sequence from that state, and the blocks are the
    restatement's from the device's words and directions.  The factors are those of the first state with delta_w = 1."""
    import torch
    from infiniteexamodels.jl_amd.barrier import AdaptiveBarrierParameter, FilterSearch, QualityFunction
    name = "opf_7"
    P = bref.barrier_point(name)
    far = (P, P["state"])
    near = next((Q, st) for label, Q, st, _, _, _ in mref.branch_cases(name) if label == "several decreases")
    with tm.objects(P) as S, FilterSearch(S.bar) as fs, AdaptiveBarrierParameter(S.par) as amu, QualityFunction(amu) as qf:
        L = S.gm._L
        k = C.c_void_p()
        assert L.iem_kkt_create(S.gm._h, 0, C.byref(k)) == 0 and L.iem_kkt_set_border(k, 1) == 0
        try:
            rng = np.random.default_rng(21)
            nanv = lambda *n: torch.full(n, NAN, dtype=torch.float64, device="cuda")
            dsz = (S.ncon, S.nvar, S.nvar, S.ncon, S.ncon)
            outs = ("w", "sigma", "dcon", "rhs2", "sol2", "alpha0", "alpha1", "rhs", "sol", "alpha", "xt", "s_t", "ct", "ft", "mt")
            bufs = dict(state=tuple(nanv(len(a)) for a in P["state"]), r=nanv(S.nvar), c=nanv(S.ncon), w=nanv(12), sigma=nanv(S.nvar), dcon=nanv(S.ncon),
                        rhs2=nanv(2, S.n), sol2=nanv(2, S.n), alpha0=nanv(2), alpha1=nanv(2), rhs=nanv(S.n), sol=nanv(S.n), alpha=nanv(2), g=T(rng.standard_normal(S.nvar)),
                        f=T([1e12]), dirs0=tuple(nanv(n) for n in dsz), dirs1=tuple(nanv(n) for n in dsz), dirs=tuple(nanv(n) for n in dsz), xt=nanv(S.nvar),
                        s_t=nanv(S.ncon), ct=nanv(S.ncon), ft=nanv(1), mt=nanv(2))
            ctl_ptr, flt_ptr = fs.device()
            cap = fs.opts["filter_capacity"]
            flt0 = np.zeros(2 * cap)
            flt0[:2] = [1e300, 1e300]
            ctl0 = np.zeros(16)
            ctl0.view(np.int64)[9], ctl0.view(np.int64)[11], ctl0.view(np.int64)[12] = 4, 1, 1
            ctl0[5], ctl0[6] = 1e-4, 1e300
            opts, aopts = mref.options(), aref.options()
            qopts = qref.options(aopts)
            blk0, ab0, qb0 = mref.fresh_block(opts), aref.fresh_block(aopts), qref.fresh_block()
            aptr, qptr = amu.device(), qf.device()
            n_wg = S.bar.info["workgroups"]
            all_dirs = lambda: bufs["dirs"] + bufs["dirs0"] + bufs["dirs1"]

            def load(case):
                Q, st_h = case
                for t, a in zip(bufs["state"], st_h):
                    t.copy_(T(a))
                bufs["r"].copy_(T(Q["r"])); bufs["c"].copy_(T(Q["c"]))
                for key in outs:
                    bufs[key].fill_(NAN)
                for t in all_dirs():
                    t.fill_(NAN)
                poke(ctl_ptr, ctl0); poke(flt_ptr, flt0); poke(S.blk, blk0); poke(aptr, ab0); poke(qptr, qb0)

            def results():
                flat = [H(t) for t in bufs["state"]] + [H(bufs[key]) for key in outs] + [H(t) for t in all_dirs()]
                return flat, peek(ctl_ptr), peek(flt_ptr, 2 * cap), peek(S.blk), peek(aptr), peek(qptr, 32)
            # the factors: the first state's matrix, sigma and dcon from terms(mu = 0)
            load(far)
            st = bufs["state"]
            jv, hv = nanv(int(S.gm.meta.nnzj)), nanv(int(S.gm.meta.nnzh))
            S.gm.jac_hess_coord(st[0], st[2], jv, hv, obj_weight=1.0)
            S.bar.terms(st, bufs["r"], bufs["c"], 0.0, out=(bufs["sigma"], bufs["dcon"], bufs["rhs"]))
            S.gm._sync_stream()
            p = lambda t: C.c_void_p(t.data_ptr())
            inertia = (C.c_int64 * 3)()
            assert L.iem_kkt_assemble_diag(k, p(hv), p(jv), p(bufs["sigma"]), p(bufs["dcon"]), DW, DC) == 0 and L.iem_kkt_factor(k, inertia) == 0
            S.bar.bind_mu(S.par); fs.bind_mu(S.par)
            expected = {}
            for label, case in (("near", near), ("far", far)):      # (the first eager sequence does the set-up)
                load(case)
                state_h = tuple(H(t) for t in bufs["state"])
                _iteration(S, fs, amu, qf, k, bufs)
                expected[label] = results()
                flat, ctl, flt, blk, ab, qb = expected[label]
                w12, sol2 = flat[7], flat[11]
                nd = len(flat) - 15
                d0 = (sol2[0], *flat[nd + 5:nd + 10])
                d1 = (sol2[1], *flat[nd + 10:nd + 15])
                Q = case[0]
                qref_blk = qref.begin(S.B, state_h, Q["r"], Q["c"], w12, ab0, aopts, qopts, n_wg)
                qref_blk = qref.section(S.B, state_h, d0, d1, qref_blk, blk0, qopts, n_wg)
                ref, aref_blk, ctl_ref = qref.update(blk0, ab0, qref_blk, w12, S.counts, opts, aopts, False, ctl0)
                print(label, "section", qref.ints(qb)[:4].tolist(), "sigma", qb[qref.BEST], "q", qb[qref.QBEST], "mu", blk[0], "tau", blk[1], "mode", mref.ints(ab)[0],
                      "alpha", flat[16].tolist(), "search status", ctl.view(np.int64)[9])
                assert same_bits(qb, qref_blk), (label, qb, qref_blk)
                assert same_bits(blk, ref) and same_bits(ab, aref_blk), label
                assert qref.ints(qb)[qref.STATUS] == qref.DONE and mref.ints(blk)[8] == mref.ITERATING and mref.ints(blk)[9] & 1
                assert np.isfinite(flat[11]).all() and np.isfinite(flat[15]).all()      # the solves gave directions
            assert not same_bits(expected["far"][3], expected["near"][3]) and not same_bits(expected["far"][5], expected["near"][5])
            load(far)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                _iteration(S, fs, amu, qf, k, bufs)
            S.gm._sync_stream()
            for label, case in (("far", far), ("near", near), ("far", far)):
                load(case)
                g.replay()
                torch.cuda.synchronize()
                got, want = results(), expected[label]
                for i, (a, b) in enumerate(zip(got[0], want[0])):
                    assert same_bits(a, b), (label, i)
                for i in range(1, 6):
                    assert same_bits(got[i], want[i]), (label, i)
            fs.bind_mu(None); S.bar.bind_mu(None)
        finally:
            torch.cuda.synchronize()
            assert L.iem_kkt_destroy(k) == 0


@pytest.mark.parametrize("name,want", [("rosenbrock", 306.4999755050365), ("ode_5x5", -12.784599900757165)])
def test_the_loop_with_the_quality_function(name, want, built):
    """tests/qf_loop.py with the rule on the device and with the restatement on the host: bitwise the same x after every iteration,
    the optimum and the error of tests/test_gpu_amu.py::test_the_loop_with_the_adaptive_rule, no failed search.  On the host alone
    (tests/test_qf.py) the restated rule takes 25 iterations on rosenbrock and 7 on ode_5x5; the counts here are printed, not
    asserted (DESIGN.md 7 f4q has them)."""
    import cases
    import qf_loop
    from infiniteexamodels.jl_amd import transcribe
    from infiniteexamodels.jl_amd.model import ExaModel
    core = transcribe.exa_core(cases.rosenbrock()[0]) if name == "rosenbrock" else cases.build_core(name)
    gm = ExaModel(core, device=0)
    try:
        res = {flag: qf_loop.solve(gm, flag, tol=1e-8) for flag in (True, False)}
        for flag, r in res.items():
            print(name, "device_rule", flag, "iterations", r["iterations"], "objective", repr(r["objective"]), "error", r["error"], "to_fixed", r["to_fixed"],
                  "to_free", r["to_free"], "searches", r["statuses"], "mu", ["%.3e" % v for v in r["mus"]], "sigma", ["%.3g" % v for v in r["sigmas"]], "modes", r["modes"],
                  "sections", r["sections"])
        a, b = res[True], res[False]
        assert a["iterations"] == b["iterations"] and len(a["iterates"]) == len(b["iterates"]) == a["iterations"]
        for i, (xa, xb) in enumerate(zip(a["iterates"], b["iterates"])):
            assert same_bits(xa, xb), i
        assert same_bits(a["mus"], b["mus"]) and same_bits(a["sigmas"], b["sigmas"]) and a["modes"] == b["modes"] and a["sections"] == b["sections"]
        assert (a["to_fixed"], a["to_free"]) == (b["to_fixed"], b["to_free"])
        for flag, r in res.items():
            assert r["failed"] == 0 and set(r["statuses"]) <= {"accepted_f", "accepted_h"}, r["statuses"]
            assert r["status"] == mref.CONVERGED and r["error"] <= 1e-8 and abs(r["objective"] - want) <= 1e-6
    finally:
        gm.close()


def test_refusals(built):
    """IEM_E_ARG before any device work: the three blocks are bitwise as before"""
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.barrier import AdaptiveBarrierParameter, BarrierLayer, FilterSearch, QualityFunction
    P = bref.barrier_point("opf_7")
    with tm.objects(P) as S, AdaptiveBarrierParameter(S.par) as amu:
        L, a = amu._handle()
        err = lambda: L.iem_last_error().decode()
        out = C.c_void_p()
        inf = float("inf")
        for bad, word in ((dict(mu_ref=0.0), "mu_ref"), (dict(mu_ref=-1.0), "mu_ref"), (dict(sigma_min=0.0), "sigma_min"), (dict(sigma_max=-1.0), "sigma_max"),
                          (dict(section_sigma_tol=0.0), "section_sigma_tol"), (dict(max_section_steps=0), "max_section_steps"), (dict(max_section_steps=17), "max_section_steps"),
                          (dict(mu_ref=inf), "finite"), (dict(sigma_min=NAN), "finite"), (dict(sigma_max=inf), "finite"), (dict(section_sigma_tol=NAN), "finite")):
            o = iemlib.QfOpts.defaults(**bad)
            assert L.iem_qf_create(a, C.byref(o), C.byref(out)) == -4 and word in err(), bad
        o = iemlib.QfOpts.defaults(); o.struct_size = 4
        assert L.iem_qf_create(a, C.byref(o), C.byref(out)) == -4 and "struct_size" in err()
        assert L.iem_qf_create(None, None, C.byref(out)) == -4 and L.iem_qf_create(a, None, None) == -4 and "null" in err()
        o = iemlib.AmuOpts.defaults(oracle=2)
        assert L.iem_amu_create(S.par._handle()[1], C.byref(o), C.byref(out)) == -4 and "oracle" in err()      # iem_amu_create keeps refusing it
        raw = C.c_void_p()
        iemlib.check(L.iem_qf_create(a, None, C.byref(raw)))      # NULL options: the defaults
        ptr = C.c_void_p()
        assert L.iem_qf_device(raw, C.byref(ptr)) == 0
        assert same_bits(peek(ptr.value, 32), qref.fresh_block())
        pattern = np.arange(32, dtype=np.float64) + 0.5
        qref.ints(pattern)[qref.STATUS] = qref.SECTION
        poke(ptr.value, pattern)
        before = (peek(S.blk), peek(amu.device()), peek(ptr.value, 32))
        d0_h, d1_h = columns(P)
        keep = [*dev(d0_h), *dev(d1_h), T(np.zeros(12))]
        st = S.st
        pair = [C.c_void_p(t.data_ptr()) for t in (st[0], st[1], st[3], st[4], st[5], st[6], *keep[:12])]
        for k in range(len(pair)):
            args = list(pair); args[k] = None
            assert L.iem_qf_alpha(raw, *args) == -4 and "null" in err(), k
            assert L.iem_qf_value(raw, *args) == -4 and "null" in err(), k
        w12 = C.c_void_p(keep[12].data_ptr())
        first = [C.c_void_p(t.data_ptr()) for t in (*st, S.r, S.c)] + [w12]
        for k in range(len(first)):
            args = list(first); args[k] = None
            assert L.iem_qf_begin(raw, *args) == -4 and "null" in err(), k
        assert L.iem_qf_update(raw, None, 0, None) == -4 and "null" in err()
        with BarrierLayer(S.gm, relax=bref.RELAX) as bar2, FilterSearch(bar2) as fs2:
            assert L.iem_qf_update(raw, w12, 0, fs2._handle()[1]) == -4 and "another barrier object" in err()
        v, u, t = iemlib.MuState(), iemlib.AmuState(), iemlib.QfState()
        v.struct_size, u.struct_size, t.struct_size = C.sizeof(iemlib.MuState), C.sizeof(iemlib.AmuState), 0
        assert L.iem_qf_state(raw, C.byref(v), C.byref(u), C.byref(t)) == -4 and "struct_size" in err()
        assert L.iem_qf_state(raw, None, C.byref(u), C.byref(t)) == -4 and L.iem_qf_state(raw, C.byref(v), C.byref(u), None) == -4 and "null" in err()
        assert all(same_bits(x, y) for x, y in zip((peek(S.blk), peek(amu.device()), peek(ptr.value, 32)), before))      # a refused call does no device work
        v.struct_size, u.struct_size, t.struct_size, t.steps = 24, 16, 16, -5
        iemlib.check(L.iem_qf_state(raw, C.byref(v), C.byref(u), C.byref(t)))
        assert (v.mu, v.tau, v.struct_size) == (0.1, 0.99, 24) and (u.mode, u.struct_size) == (0, 16)
        assert (t.status, t.steps, t.struct_size) == (qref.SECTION, -5, 16)      # short structs receive their heads only
        iemlib.check(L.iem_qf_destroy(raw))
        assert L.iem_qf_destroy(None) == 0
        with pytest.raises(TypeError):
            QualityFunction(amu, kappa=1.0)
        with QualityFunction(amu, sigma_max=7.0, max_section_steps=3) as qf:
            assert qf.opts["sigma_max"] == 7.0 and qf.pairs == 7 and qf.state()["section"]["status_name"] == "idle"
            qf.update(keep[12])      # an idle section: UNUSABLE, whatever the words
            assert qf.state()["status_name"] == "unusable"
    with pytest.raises(iemlib.IemError, match="closed"):
        qf.reset()
