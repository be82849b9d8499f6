"""The adaptive barrier parameter object (iem_amu_*, csrc/iem_amu_device.h) on the MI355X.

BITWISE against tests/amu_reference.py: words 1–3 of iem_amu_probe and both blocks (and a search's control block) after
iem_amu_update on every entry of `branch_cases`, for both oracles.  Word 0 of the probe carries the bits of
amu_reference.probe_sum — the restatement in the DEVICE'S ORDER (barrier_reference.device_sum) on the object's own grid of
info["workgroups"] workgroups — repeats bit for bit, and with zero directions and alpha = (1, 1) carries the bits of word 9 of
iem_mu_error on the same state: the summation order is the existing kernel's.  One iteration — the affine solve, the probe and the
adaptive update included — captured once replays at two states; tests/amu_loop.py converges with the rule on the device and with
the restatement on the host through bitwise the same iterates.

Shapes: those of tests/test_gpu_mu.py, whose helpers this file shares — opf_7 (two workgroups), quadrotor_100 (several workgroups:
the last-arrival path; nz = 0), `maratos` (every row an equality) and the two big shapes of barrier_reference.big_point on 4096
workgroups: quadrotor(27 000) (nvar + ncon > 2²⁰: the grid-stride loop runs a second trip, rows only) and quadrotor(60 000) (nvar >
2²⁰: three trips, the second across the nvar seam — asserted and printed)."""
import ctypes as C
import math

import numpy as np
import pytest

import amu_reference as aref
import barrier_reference as bref
import mu_reference as mref
import test_gpu_mu as tm

pytestmark = pytest.mark.gpu
NAN = float("nan")
PAD = 5
WRONG_MU, WRONG_TAU = 123.0, 0.5
DW, DC = 1.0, 1e-8
T, H, same_bits, peek, poke = tm.T, tm.H, tm.same_bits, tm.peek, tm.poke


def probe(S, amu, sol, dirs, alpha, st=None):
    """iem_amu_probe into a NaN-poisoned buffer: the four words on the host, the padding checked"""
    import torch
    buf = torch.full((4 + PAD,), NAN, dtype=torch.float64, device="cuda")
    amu.probe(st if st is not None else S.st, sol, dirs, alpha, out=buf[:4])
    h = H(buf)
    assert np.isnan(h[4:]).all(), "padding touched"
    return h[:4]


directions = aref.directions


@pytest.mark.parametrize("name", tm.SHAPES)
def test_probe_words(name, built):
    from infiniteexamodels.jl_amd.barrier import AdaptiveBarrierParameter
    P = tm.point(name)
    with tm.objects(P) as S, AdaptiveBarrierParameter(S.par) as amu:
        B, st_h = S.B, P["state"]
        sol_h, dirs_h, alpha_h = directions(P)
        sol, dirs, alpha = T(sol_h), tuple(T(d) for d in dirs_h), T(alpha_h)
        q = probe(S, amu, sol, dirs, alpha)
        p, nan, ap, ad = aref.probe_words(B, st_h, sol_h, dirs_h, alpha_h)
        n_wg = S.bar.info["workgroups"]
        assert n_wg == min(-(-S.n // 256), 4096)
        if name in tm.BIG:
            tm.big_facts(name, S)
        q0 = aref.probe_sum(B, st_h, sol_h, dirs_h, alpha_h, n_wg)
        print(name, "workgroups", n_wg, "nz", S.counts[1], "alpha", alpha_h.tolist(), "q0", repr(q[0]), "device order", repr(float(q0)), "fsum", math.fsum(p), "q1", q[1])
        assert len(p) == S.counts[1] and nan == 0.0
        assert same_bits(q[1:], [nan, ap, ad]), q
        assert same_bits(q[0], q0), (q[0], q0)
        assert same_bits(probe(S, amu, sol, dirs, alpha), q)      # the same bits again: the sum has one order
        # zero directions, alpha = (1, 1): the sum of the complementarity products, in the order of iem_mu_error's word 9
        zero = tuple(T(np.zeros(len(d))) for d in dirs_h)
        q0 = probe(S, amu, T(np.zeros(S.n)), zero, T([1.0, 1.0]))
        w = tm.words(S)
        assert same_bits(q0, [w[9], 0.0, 1.0, 1.0]), (q0, w[9])
        # NaN wherever nothing may be read — absent bounds, equality rows, dy, variables and rows without any bound: the same bits
        anyx, anys = B["hasL"] | B["hasU"], B["gL"] | B["gU"]
        sol_n = sol_h.copy()
        sol_n[:S.nvar][~anyx] = NAN
        sol_n[S.nvar:] = NAN
        ds, dzL, dzU, dvL, dvU = (d.copy() for d in dirs_h)
        ds[~anys] = NAN; dzL[~B["hasL"]] = NAN; dzU[~B["hasU"]] = NAN; dvL[~B["gL"]] = NAN; dvU[~B["gU"]] = NAN
        st_n = [a.copy() for a in st_h]
        st_n[0][~anyx] = NAN; st_n[1][~anys] = NAN; st_n[2][:] = NAN
        st_n[3][~B["hasL"]] = NAN; st_n[4][~B["hasU"]] = NAN; st_n[5][~B["gL"]] = NAN; st_n[6][~B["gU"]] = NAN
        assert not anys[B["eq"]].any()      # (an equality row has no bound of its own: its entries are among the poisoned)
        assert same_bits(probe(S, amu, T(sol_n), tuple(T(d) for d in (ds, dzL, dzU, dvL, dvU)), alpha, st=tuple(T(a) for a in st_n)), q)
        if S.counts[1] == 0:
            assert same_bits(q, [0.0, 0.0, alpha_h[0], alpha_h[1]])
            return
        # a NaN in a direction at a present bound is counted
        where = [(1, B["hasL"]), (2, B["hasU"]), (3, B["gL"]), (4, B["gU"])]
        k, on = next((k, on) for k, on in where if on.any())
        i = int(np.flatnonzero(on)[-1])
        bad = [d.copy() for d in dirs_h]
        bad[k][i] = NAN
        qb = probe(S, amu, sol, tuple(T(d) for d in bad), alpha)
        assert same_bits(qb[1:], [1.0, ap, ad]) and np.isnan(qb[0]), qb
        assert aref.probe_words(B, st_h, sol_h, tuple(bad), alpha_h)[1] == 1.0


@pytest.mark.parametrize("name", ["opf_7", "maratos"])
@pytest.mark.parametrize("oracle", [aref.PROBING, aref.LOQO])
def test_update_branches(oracle, name, built):
    """both blocks and the search's control block are the restatement's on every entry of `branch_cases` (maratos: the nz = 0
    branches); a search's words 11, 12 are cleared exactly when the bits of mu changed, its other words and its filter never"""
    from infiniteexamodels.jl_amd.barrier import AdaptiveBarrierParameter, BarrierParameter, FilterSearch
    P = tm.point(name)
    with tm.objects(P) as S, FilterSearch(S.bar) as fs:
        cases = aref.branch_cases(oracle, S.counts)
        assert len(cases) >= (5 if S.counts[1] == 0 else 18)
        for case in cases:
            opts, aopts, label = case["opts"], case["aopts"], case["label"]
            over = {k: v for k, v in opts.items() if v != mref.options()[k]}
            aover = {k: v for k, v in aopts.items() if v != aref.OPTS[k]}
            with BarrierParameter(S.bar, **over) as par, AdaptiveBarrierParameter(par, **aover) as amu:
                ptr, aptr = par.device(), amu.device()
                assert same_bits(peek(aptr), aref.fresh_block(aopts)), label
                poke(ptr, case["blk"]); poke(aptr, case["ab"])
                ctl_ptr, flt_ptr, ctl, flt = tm.pattern_search(S, fs)
                wd = T(case["w"])
                qd = T(case["probe"]) if case["probe"] is not None else None
                amu.update(wd, qd, force_fixed=case["force_fixed"], search=fs)
                blk, ab = peek(ptr), peek(aptr)
                ref, aref_blk, ctl_ref = aref.update(case["blk"], case["ab"], case["w"], case["probe"], S.counts, opts, aopts, case["force_fixed"], ctl)
                iw, ia = mref.ints(blk), mref.ints(ab)
                print(name, aref.options(oracle=oracle)["oracle"], label, "mu", blk[0], "tau", blk[1], "E0", blk[3], "status", iw[8], "flags", iw[9], "decreases", iw[10],
                      "mode", ia[0], "mu_max", ab[1], "refs", ia[2], "sigma", ab[8], "avg", ab[9])
                assert same_bits(blk, ref), (label, blk, ref)
                assert same_bits(ab, aref_blk), (label, ab, aref_blk)
                assert same_bits(peek(ctl_ptr), ctl_ref) and same_bits(peek(flt_ptr, len(flt)), flt), label
                assert same_bits(ctl_ref[11:13], [0.0, 0.0]) == bool(iw[9] & 1) == (not same_bits(blk[0], case["blk"][0])), label
                s = amu.state()
                assert same_bits([s[k] for k in ("mu", "tau", "zeta", "e0", "e_mu", "e_d", "e_p", "e_c0")], blk[:8])
                assert (s["status"], s["flags"], s["decreases"], s["updates"]) == tuple(iw[8:12]) and s["changed"] == bool(iw[9] & 1)
                assert (s["mode"], s["to_fixed"], s["to_free"], s["oracle"]) == (ia[0], ia[11], ia[12], oracle) and len(s["refs"]) == ia[2]
                assert same_bits([s["mu_max"], *s["refs"], s["mu_oracle"], s["sigma"], s["avg"], s["m_aff"]], [ab[1], *ab[3:3 + ia[2]], *ab[7:11]])
                # without a search: the same blocks, the search untouched; then reset: the own block is fresh, the other stays
                poke(ptr, case["blk"]); poke(aptr, case["ab"])
                amu.update(wd, qd, force_fixed=case["force_fixed"])
                assert same_bits(peek(ptr), ref) and same_bits(peek(aptr), aref_blk) and same_bits(peek(ctl_ptr), ctl_ref), label
                amu.reset()
                assert same_bits(peek(aptr), aref.fresh_block(aopts)) and same_bits(peek(ptr), ref), label


def _iteration(S, fs, amu, k, bufs):
    """error, unbind, affine terms / solve / step / probe, bind, update, terms, solve, step, begin, one rung, barrier update — on the
    factors the solver object holds; the host's mu and tau are wrong wherever an object is bound"""
    b, gm, L = S.bar, S.gm, S.gm._L
    st = bufs["state"]
    p = lambda t: C.c_void_p(t.data_ptr())

    def solve(rhs, sol):
        gm._sync_stream()
        assert L.iem_kkt_solve_refined_diag(k, p(st[0]), p(st[2]), 1.0, p(bufs["sigma"]), p(bufs["dcon"]), DW, DC, 1, p(rhs), S.n, p(sol), S.n, 1, None) == 0
    S.par.error(st, bufs["r"], bufs["c"], out=bufs["w"])
    with amu.affine(b, fs):
        b.terms(st, bufs["r"], bufs["c"], 0.0, out=(bufs["sigma"], bufs["dcon"], bufs["rhs_a"]))
        solve(bufs["rhs_a"], bufs["sol_a"])
        b.step(st, bufs["sol_a"], 0.0, 1.0, out=bufs["dirs_a"], alpha=bufs["alpha_a"])
        amu.probe(st, bufs["sol_a"], bufs["dirs_a"], bufs["alpha_a"], out=bufs["q"])
    amu.update(bufs["w"], bufs["q"], search=fs)
    b.terms(st, bufs["r"], bufs["c"], WRONG_MU, out=(bufs["sigma"], bufs["dcon"], bufs["rhs"]))
    solve(bufs["rhs"], bufs["sol"])
    b.step(st, bufs["sol"], WRONG_MU, WRONG_TAU, out=bufs["dirs"], alpha=bufs["alpha"])
    fs.begin(st, bufs["g"], bufs["sol"], bufs["dirs"][0], bufs["f"], bufs["w"][:8], bufs["alpha"], WRONG_MU)
    fs.trial(st, bufs["sol"], bufs["dirs"][0], bufs["xt"], bufs["s_t"])
    gm.obj_device(bufs["xt"], out=bufs["ft"])
    gm.cons(bufs["xt"], bufs["ct"])
    b.merit(bufs["xt"], bufs["s_t"], bufs["ct"], out=bufs["mt"])
    fs.accept(bufs["ft"], bufs["mt"], WRONG_MU, bufs["alpha"])
    b.update(st, bufs["sol"], bufs["dirs"], bufs["alpha"], WRONG_MU)


def test_one_graph_with_the_adaptive_rule(built):
    """ONE captured iteration (no synchronisation inside: the capture would refuse it) replayed from two states: every buffer, both
    blocks, the search's block and its filter are bitwise the eager sequence from that state, and the blocks are the restatement's
    from the device's sixteen words.  The factors are those of the first state with delta_w = 1 — any fixed factors serve."""
    import torch
    from infiniteexamodels.jl_amd.barrier import AdaptiveBarrierParameter, FilterSearch
    name = "opf_7"
    P = bref.barrier_point(name)
    far = (P, P["state"])
    near = next((Q, st) for label, Q, st, _, _, _ in mref.branch_cases(name) if label == "several decreases")
    with tm.objects(P) as S, FilterSearch(S.bar) as fs, AdaptiveBarrierParameter(S.par) as amu:
        L = S.gm._L
        k = C.c_void_p()
        assert L.iem_kkt_create(S.gm._h, 0, C.byref(k)) == 0 and L.iem_kkt_set_border(k, 1) == 0
        try:
            rng = np.random.default_rng(21)
            nanv = lambda n: torch.full((n,), NAN, dtype=torch.float64, device="cuda")
            dsz = (S.ncon, S.nvar, S.nvar, S.ncon, S.ncon)
            outs = ("w", "q", "sigma", "dcon", "rhs_a", "sol_a", "alpha_a", "rhs", "sol", "alpha", "xt", "s_t", "ct", "ft", "mt")
            bufs = dict(state=tuple(nanv(len(a)) for a in P["state"]), r=nanv(S.nvar), c=nanv(S.ncon), w=nanv(12), q=nanv(4), sigma=nanv(S.nvar), dcon=nanv(S.ncon),
                        rhs_a=nanv(S.n), sol_a=nanv(S.n), alpha_a=nanv(2), rhs=nanv(S.n), sol=nanv(S.n), alpha=nanv(2), g=T(rng.standard_normal(S.nvar)), f=T([1e12]),
                        dirs_a=tuple(nanv(n) for n in dsz), dirs=tuple(nanv(n) for n in dsz), xt=nanv(S.nvar), s_t=nanv(S.ncon), ct=nanv(S.ncon), ft=nanv(1), mt=nanv(2))
            ctl_ptr, flt_ptr = fs.device()
            cap = fs.opts["filter_capacity"]
            flt0 = np.zeros(2 * cap)
            flt0[:2] = [1e300, 1e300]
            ctl0 = np.zeros(16)
            ctl0.view(np.int64)[9], ctl0.view(np.int64)[11], ctl0.view(np.int64)[12] = 4, 1, 1
            ctl0[5], ctl0[6] = 1e-4, 1e300
            opts, aopts = mref.options(), aref.options()
            blk0, ab0 = mref.fresh_block(opts), aref.fresh_block(aopts)
            aptr = amu.device()

            def load(case):
                Q, st_h = case
                for t, a in zip(bufs["state"], st_h):
                    t.copy_(T(a))
                bufs["r"].copy_(T(Q["r"])); bufs["c"].copy_(T(Q["c"]))
                for key in outs:
                    bufs[key].fill_(NAN)
                for t in bufs["dirs"] + bufs["dirs_a"]:
                    t.fill_(NAN)
                poke(ctl_ptr, ctl0); poke(flt_ptr, flt0); poke(S.blk, blk0); poke(aptr, ab0)

            def results():
                flat = [H(t) for t in bufs["state"]] + [H(bufs[key]) for key in outs] + [H(t) for t in bufs["dirs"] + bufs["dirs_a"]]
                return flat, peek(ctl_ptr), peek(flt_ptr, 2 * cap), peek(S.blk), peek(aptr)
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
            S.bar.bind_mu(S.par); fs.bind_mu(S.par)
            expected = {}
            for label, case in (("near", near), ("far", far)):      # (the first eager sequence does the set-up)
                load(case)
                _iteration(S, fs, amu, k, bufs)
                expected[label] = results()
                flat, ctl, flt, blk, ab = expected[label]
                w12, q4 = flat[7], flat[8]
                ref, aref_blk, ctl_ref = aref.update(blk0, ab0, w12, q4, S.counts, opts, aopts, False, ctl0)
                print(label, "probe", q4.tolist(), "mu", blk[0], "tau", blk[1], "sigma", ab[8], "avg", ab[9], "mode", mref.ints(ab)[0], "alpha", flat[16].tolist(),
                      "search status", ctl.view(np.int64)[9])
                assert same_bits(blk, ref) and same_bits(ab, aref_blk), label
                assert mref.ints(blk)[8] == mref.ITERATING and mref.ints(blk)[9] & 1 and q4[1] == 0.0 and q4[2] > 0.0 and q4[3] > 0.0
                assert np.isfinite(flat[12]).all() and np.isfinite(flat[15]).all()      # both solves gave a direction
            assert not same_bits(expected["far"][0][0], P["state"][0]) or expected["far"][0][16][0] == 0.0      # the far iteration took a step (or its search refused)
            assert not same_bits(expected["far"][3], expected["near"][3])
            load(far)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                _iteration(S, fs, amu, k, bufs)
            S.gm._sync_stream()
            for label, case in (("far", far), ("near", near), ("far", far)):
                load(case)
                g.replay()
                torch.cuda.synchronize()
                got, want = results(), expected[label]
                for i, (a, b) in enumerate(zip(got[0], want[0])):
                    assert same_bits(a, b), (label, i)
                for i in range(1, 5):
                    assert same_bits(got[i], want[i]), (label, i)
            fs.bind_mu(None); S.bar.bind_mu(None)
        finally:
            torch.cuda.synchronize()
            assert L.iem_kkt_destroy(k) == 0


_monotone = {}


@pytest.mark.parametrize("oracle", [aref.PROBING, aref.LOQO])
@pytest.mark.parametrize("name,want", [("rosenbrock", 306.4999755050365), ("ode_5x5", -12.784599900757165)])
def test_the_loop_with_the_adaptive_rule(name, want, oracle, built):
    """tests/amu_loop.py with the rule on the device and with the restatement on the host: bitwise the same x after every iteration,
    the optimum and the error of tests/test_gpu_mu.py::test_the_loop_with_mu_on_the_device, no failed search.  Iteration counts, the
    mu sequence and the mode switches are printed beside the count of the monotone rule (computed once per model; not asserted
    against one another — DESIGN.md 7 f4a has them)."""
    import amu_loop
    import cases
    import mu_loop
    from infiniteexamodels.jl_amd import transcribe
    from infiniteexamodels.jl_amd.model import ExaModel
    core = transcribe.exa_core(cases.rosenbrock()[0]) if name == "rosenbrock" else cases.build_core(name)
    gm = ExaModel(core, device=0)
    try:
        if name not in _monotone:
            mono = mu_loop.solve(gm, device_mu=True, tol=1e-8)
            _monotone[name] = (mono["iterations"], mono["decreases"])
        print(name, "monotone rule: iterations", _monotone[name][0], "decreases", _monotone[name][1])
        res = {flag: amu_loop.solve(gm, flag, oracle, tol=1e-8) for flag in (True, False)}
        for flag, r in res.items():
            print(name, ("probing", "loqo")[oracle], "device_rule", flag, "iterations", r["iterations"], "objective", repr(r["objective"]), "error", r["error"],
                  "to_fixed", r["to_fixed"], "to_free", r["to_free"], "searches", r["statuses"], "mu", ["%.3e" % v for v in r["mus"]], "modes", r["modes"])
            assert r["failed"] == 0 and set(r["statuses"]) <= {"accepted_f", "accepted_h"}, r["statuses"]
            assert r["status"] == mref.CONVERGED and r["error"] <= 1e-8 and abs(r["objective"] - want) <= 1e-6
        a, b = res[True], res[False]
        assert a["iterations"] == b["iterations"] and len(a["iterates"]) == len(b["iterates"]) == a["iterations"]
        for i, (xa, xb) in enumerate(zip(a["iterates"], b["iterates"])):
            assert same_bits(xa, xb), i
        assert same_bits(a["mus"], b["mus"]) and a["modes"] == b["modes"] and (a["to_fixed"], a["to_free"]) == (b["to_fixed"], b["to_free"])
    finally:
        gm.close()


def test_refusals(built):
    from infiniteexamodels.jl_amd import lib as iemlib
    from infiniteexamodels.jl_amd.barrier import AdaptiveBarrierParameter, BarrierLayer, BarrierParameter, FilterSearch
    P = bref.barrier_point("opf_7")
    with tm.objects(P) as S:
        L, par = S.par._handle()
        err = lambda: L.iem_last_error().decode()
        out = C.c_void_p()
        inf = float("inf")
        for bad, word in ((dict(oracle=2), "oracle"), (dict(oracle=-1), "oracle"), (dict(sigma_max=0.0), "sigma_max"), (dict(mu_min=0.0), "mu_min"), (dict(mu_min=-1e-9), "mu_min"),
                          (dict(mu_max_fact=0.0), "mu_max_fact"), (dict(init_factor=0.0), "init_factor"), (dict(red_fact=0.0), "red_fact"), (dict(red_fact=1.0), "red_fact"),
                          (dict(refs_max=0), "refs_max"), (dict(refs_max=5), "refs_max"), (dict(sigma_max=inf), "finite"), (dict(mu_min=NAN), "finite"),
                          (dict(red_fact=NAN), "finite"), (dict(init_factor=inf), "finite")):
            o = iemlib.AmuOpts.defaults(**bad)
            assert L.iem_amu_create(par, C.byref(o), C.byref(out)) == -4 and word in err(), bad
        o = iemlib.AmuOpts.defaults(); o.struct_size = 4
        assert L.iem_amu_create(par, C.byref(o), C.byref(out)) == -4 and "struct_size" in err()
        assert L.iem_amu_create(None, None, C.byref(out)) == -4 and L.iem_amu_create(par, None, None) == -4 and "null" in err()
        raw = C.c_void_p()
        iemlib.check(L.iem_amu_create(par, None, C.byref(raw)))      # NULL options: the defaults
        ptr = C.c_void_p()
        assert L.iem_amu_device(raw, C.byref(ptr)) == 0
        assert same_bits(peek(ptr.value), aref.fresh_block(aref.options()))
        mu_before, own_before = peek(S.blk), peek(ptr.value)
        sol_h, dirs_h, alpha_h = directions(P)
        keep = [T(sol_h), *(T(d) for d in dirs_h), T(alpha_h), T(np.zeros(4)), T(np.zeros(12))]
        st = S.st
        ptrs = [C.c_void_p(t.data_ptr()) for t in (st[0], st[1], st[3], st[4], st[5], st[6], *keep[:8])]
        for k in range(len(ptrs)):
            a = list(ptrs); a[k] = None
            assert L.iem_amu_probe(raw, *a) == -4 and "null" in err(), k
        w12, q4 = C.c_void_p(keep[8].data_ptr()), C.c_void_p(keep[7].data_ptr())
        assert L.iem_amu_update(raw, None, q4, 0, None) == -4 and "null" in err()
        assert L.iem_amu_update(raw, w12, None, 0, None) == -4 and "probing" in err()
        with BarrierLayer(S.gm, relax=bref.RELAX) as bar2, FilterSearch(bar2) as fs2:
            assert L.iem_amu_update(raw, w12, q4, 0, fs2._handle()[1]) == -4 and "another barrier object" in err()
        v, u = iemlib.MuState(), iemlib.AmuState()
        v.struct_size, u.struct_size = C.sizeof(iemlib.MuState), 0
        assert L.iem_amu_state(raw, C.byref(v), C.byref(u)) == -4 and "struct_size" in err()
        assert L.iem_amu_state(raw, None, C.byref(u)) == -4 and L.iem_amu_state(raw, C.byref(v), None) == -4 and "null" in err()
        v.struct_size, u.struct_size, u.refs_count = 24, 16, -5
        iemlib.check(L.iem_amu_state(raw, C.byref(v), C.byref(u)))
        assert (v.mu, v.tau, v.struct_size) == (0.1, 0.99, 24) and (u.mode, u.refs_count, u.struct_size) == (0, -5, 16)      # short structs receive their heads only
        assert same_bits(peek(S.blk), mu_before) and same_bits(peek(ptr.value), own_before)      # a refused call does no device work
        iemlib.check(L.iem_amu_destroy(raw))
        assert L.iem_amu_destroy(None) == 0
        with pytest.raises(TypeError):
            AdaptiveBarrierParameter(S.par, kappa=1.0)
        with AdaptiveBarrierParameter(S.par, oracle="loqo") as amu:
            assert amu.opts["oracle"] == aref.LOQO and amu.state()["oracle_name"] == "loqo" and amu.state()["mode_name"] == "free"
            amu.update(keep[8])      # LOQO takes no probe: words of zero are E(0) = 0 <= tol
            assert amu.state()["status_name"] == "converged"
    with pytest.raises(iemlib.IemError, match="closed"):
        amu.reset()
