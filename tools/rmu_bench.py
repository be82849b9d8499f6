#!/usr/bin/env python3
"""What the restoration phase's barrier parameter on the device (iem_rmu_*) and the bound restoration (iem_resto_bind_mu) cost.

  rmu_error, resto_error          µs per call on the same state, with both algorithmic byte counts: rmu_error reads what resto_error
                                  reads, once, and carries six candidates' maxima through it
  enter, update                   µs per call of the one-workgroup kernels (update on the words of the state)
  trigger, trigger_decided        iem_rmu_trigger on a SEARCHING search whose step length lies above alpha_min (every call evaluates alpha_min, none
                                  fires: the search is armed in front of each block) and on a search that is decided already (the early return)
  rule_0, host_rule_0             wall clock, µs, of "restoration rule + read-back" where the words of the state decide (`decreases` in the output; none at most sizes): rmu_error + rmu_update + rmu_state
                                  against the host sequence of tests/resto_loop.py — resto.error + a read-back of the eight words, once,
                                  + resto.state()
  rule_2, host_rule_2             the same with TWO decreases: the device sequence is the same three calls (update is fed hand-built
                                  words that decide two decreases; the block is reset in front, untimed); the host sequence runs
                                  resto.error + read-back three times (two passes that decrease, one that stops)
  iteration_unbound, graph_bound  one restoration iteration — eval_residual(0), the rule, jac_hess_coord(0), terms, assemble, factor_async,
                                  refined solve, step, merit(0), begin, one rung (trial, cons, merit(1), accept, trigger), update (1e-12),
                                  obj, cons, barrier_merit, check — eager and unbound (with resto.error in the rule's place; the objects
                                  are unbound in front of its blocks and bound in front of the others) against bound and captured as ONE
                                  graph, replayed

The sizes and the method of tools/resto_bench.py: per case one child process under its own `timeout` (the parent never opens the GPU
and stops at the first child that fails); every call warmed, then blocks of back-to-back calls between ONE event pair, `--repeats`
blocks each, the calls taking turns; median, minimum and maximum per call over the blocks.  The wall-clock figures are medians over
`--repeats` blocks of `--block` sequences, each of which ends in its own synchronisation.  No duration existed for these calls before
this tool: it reports and sets no threshold.  The launches sit near the launch floor, and back-to-back calls on the same buffers run
at cache rates.

  python tools/rmu_bench.py --out profiles/rmu.json
  python tools/rmu_bench.py --case opf_10000          (one case, JSON on stdout)
"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ("pandemic_110_128", "opf_10000", "quadrotor_16000", "quadrotor_100000")
MODELS = {"pandemic_110_128": "workloads.pandemic(110, 128)", "opf_10000": "workloads.opf(10000)", "quadrotor_16000": "workloads.quadrotor(16000)",
          "quadrotor_100000": "workloads.quadrotor(100000)"}
MU, TAU, RELAX, DW, DC, RHO, TINY = 0.1, 0.99, 1e-8, 1e-2, 1e-6, 1000.0, 1e-12


def one(case, block, repeats):
    import ctypes as C
    import numpy as np
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib, transcribe, workloads
    from infiniteexamodels.jl_amd.barrier import BarrierLayer, FilterSearch, Restoration, RestorationParameter
    from infiniteexamodels.jl_amd.kkt_chain import KKTObject
    from infiniteexamodels.jl_amd.model import ExaModel
    gm = ExaModel(transcribe.exa_core(eval(MODELS[case], {"workloads": workloads})), device=0)
    meta = gm.meta
    n, m = int(meta.nvar), int(meta.ncon)
    lvar, uvar, lcon, ucon = (np.asarray(a, dtype=np.float64) for a in (meta.lvar, meta.uvar, meta.lcon, meta.ucon))
    parts, fx, fc, info = iemlib.barrier_analyse(lvar, uvar, lcon, ucon, RELAX)
    rng = np.random.default_rng(0)
    hasL, hasU, gL, gU = (fx & 1) > 0, (fx & 2) > 0, (fc & 1) > 0, (fc & 2) > 0

    def inside(v, lo, hi, a, b):
        with np.errstate(invalid="ignore"):
            v = np.where(a & b, lo + rng.uniform(0.05, 0.95, len(v)) * (hi - lo), v)
            v = np.where(a & ~b, lo + 10.0 ** rng.uniform(-2, 1, len(v)), v)
            return np.where(b & ~a, hi - 10.0 ** rng.uniform(-2, 1, len(v)), v)
    x = inside(np.asarray(meta.x0, dtype=np.float64) + 0.1 * rng.standard_normal(n), parts["xl"], parts["xu"], hasL, hasU)
    T = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")
    new = lambda k: torch.empty(k, dtype=torch.float64, device="cuda")
    zeros = lambda k: torch.zeros(k, dtype=torch.float64, device="cuda")
    xd, yd = T(x), T(0.1 * rng.standard_normal(m))
    f0, cd, rd = gm.eval_residual(xd, yd)
    s = inside(cd.cpu().numpy(), parts["rl"], parts["ru"], gL, gU)
    mult = lambda k: T(10.0 ** rng.uniform(-2, 2, k))
    state = (xd, T(s), yd, mult(n), mult(n), mult(m), mult(m))
    mi = info["n_ineq"]
    # algorithmic bytes, counted as tools/resto_bench.py counts resto_error's (every bound counted as present): the flags, then 8-byte words
    b_error = {"read": 8 * (8 * n + 7 * m + 7 * mi) + n + m, "written": 8 * 8}
    b_rmu = {"read": 8 * (8 * n + 7 * m + 7 * mi) + n + m + 8 * 3, "written": 8 * 32}
    res = {"case": case, "model": MODELS[case], "device": torch.cuda.get_device_name(0), "repeats": repeats, "calls_per_block": block, **info,
           "alg_bytes_per_call": {"resto_error": b_error, "rmu_error": b_rmu}}

    with BarrierLayer(gm, relax=RELAX) as bar, KKTObject(gm) as kkt, FilterSearch(bar) as fs, Restoration(fs, rho=RHO) as resto, RestorationParameter(resto) as rp:
        counts_r = (info["ncon"], info["nz"] + 2 * info["ncon"])
        err8 = bar.error(state, rd, cd, MU)
        mu = max(MU, float(err8[2]))
        zeta = math.sqrt(mu)
        res["mu"], res["zeta"] = mu, zeta
        jv, hv = new(int(meta.nnzj)), new(int(meta.nnzh))
        sigma, dcon, rhs, sol = new(n), new(m), new(n + m), new(n + m)
        dirs, alpha, tiny = (zeros(m), new(n), new(n), zeros(m), zeros(m)), new(2), T([TINY, TINY])
        xt, st, ct, f1, m2, m3, mt3, e8, w32 = new(n), zeros(m), new(m), new(1), new(2), new(3), new(3), new(8), new(32)
        inertia = torch.zeros(3, dtype=torch.int64, device="cuda")
        kkt.set_border(1)
        L, k = kkt._handle()
        p = lambda t: C.c_void_p(t.data_ptr())
        rp.enter(err8, MU)      # mu_R = max(MU, max |inf|): the block holds what the unbound calls get as host doubles
        resto.enter(state, cd, mu)
        torch.cuda.synchronize()
        first = rp.state()
        assert first["mu"] == mu and first["zeta"] == zeta and first["status"] == 0, first
        # hand-built words on which the rule decides exactly two decreases (the layout of iem_rmu_error; sd = sc = 1)
        two = np.zeros(32)
        cand = [mu]
        for _ in range(5):
            cand.append(max(1e-11, min(0.2 * cand[-1], cand[-1] * math.sqrt(cand[-1]))))
        two[4], two[5] = 1.0, 2.0
        for q in range(6):
            two[12 + 3 * q], two[13 + 3 * q], two[14 + 3 * q] = cand[q], (5.0 if q < 2 else 20.0) * cand[q], 0.0
        two[0] = two[13]
        w_two = T(two)

        def factor_and_solve():
            kkt.assemble(hv, jv, sigma, DW, DC, dcon=dcon, at=(xd, yd, 0.0))
            iemlib.check(L.iem_kkt_factor_async(k, p(inertia)))
            iemlib.check(L.iem_kkt_solve_refined_diag(k, p(xd), p(yd), 0.0, p(sigma), p(dcon), DW, DC, 1, p(rhs), n + m, p(sol), n + m, 1, None))

        def iteration(bound):
            a_mu, a_tau, a_zeta = (0.0, 1.0, 0.0) if bound else (mu, TAU, zeta)
            gm.eval_residual(xd, yd, 0.0, c=cd, out=rd, obj=f1)
            if bound:
                rp.error(state, rd, cd, out=w32)
                rp.update(w32)
            else:
                resto.error(state, rd, cd, mu, zeta, out=e8)
            gm.jac_hess_coord(xd, yd, jv, hv, obj_weight=0.0)
            resto.terms(state, rd, cd, a_mu, a_zeta, out=(sigma, dcon, rhs))
            factor_and_solve()
            resto.step(state, sol, a_mu, a_tau, a_zeta, out=dirs, alpha=alpha)
            resto.merit(0, xd, state[1], cd, a_zeta, out=m3)
            resto.begin(state, sol, dirs[0], m3, alpha, a_mu, a_zeta)
            resto.trial(state, sol, dirs[0], xt, st)
            gm.cons(xt, ct)
            resto.merit(1, xt, st, ct, a_zeta, out=mt3)
            resto.inner.accept(mt3[0:1], mt3[1:3], a_mu, alpha)
            if bound:
                rp.trigger(1, alpha)
            resto.update(state, sol, dirs, tiny, a_mu)
            gm.obj_device(xd, out=f1)
            gm.cons(xd, cd)
            bar.merit(xd, state[1], cd, out=m2)
            resto.check(f1, m2, MU)

        def bind(on):      # (no launch: a pointer in the handle; the first bind has loaded the bound code object)
            resto.bind_mu(rp if on else None)
            resto.inner.bind_mu(rp.inner_mu if on else None)

        def prepare():
            bind(False)
            rp.inner_mu.reset(mu)
            resto.enter(state, cd, mu)
            resto.step(state, sol, mu, TAU, zeta, out=dirs, alpha=alpha)
        iteration(False)
        torch.cuda.synchronize()
        res["inertia"] = inertia.tolist()
        g0, a_live, a_tiny, a_out = zeros(n), T([0.5, 1.0]), T([1e-30, 1.0]), new(2)

        def arm_trigger(decided):
            """the ORIGINAL search's block in front of a block of trigger calls: SEARCHING with a step length far above alpha_min (every call
            evaluates alpha_min and does not fire), or — decided — FAILED by a first trigger on a step length of 1e-30 (every call returns early)"""
            fs.begin(state, g0, sol, dirs[0], f1, err8, a_tiny if decided else a_live, MU)
            if decided:
                rp.trigger(0, a_out)
        calls = {"rmu_error": lambda: rp.error(state, rd, cd, out=w32), "resto_error": lambda: resto.error(state, rd, cd, mu, zeta, out=e8),
                 "enter": lambda: rp.enter(err8, MU), "update": lambda: rp.update(w32), "trigger": lambda: rp.trigger(0, a_out), "trigger_decided": lambda: rp.trigger(0, a_out),
                 "iteration_unbound": lambda: iteration(False)}
        arm = {"trigger": lambda: arm_trigger(False), "trigger_decided": lambda: arm_trigger(True), "iteration_unbound": lambda: bind(False)}

        def timed(names, blk):
            for nm in names:
                prepare()
                arm.get(nm, lambda: None)()
                for _ in range(3):
                    calls[nm]()
            torch.cuda.synchronize()
            us = {nm: [] for nm in names}
            for _ in range(repeats):
                for nm in names:
                    prepare()
                    arm.get(nm, lambda: None)()
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(blk):
                        calls[nm]()
                    e1.record(); torch.cuda.synchronize()
                    us[nm].append(1e3 * e0.elapsed_time(e1) / blk)
            return {nm: {"us_median": float(np.median(v)), "us_min": min(v), "us_max": max(v)} for nm, v in us.items()}
        prepare()
        rp.error(state, rd, cd, out=w32)
        torch.cuda.synchronize()
        res["us_per_call"] = timed(["rmu_error", "resto_error", "enter", "update", "trigger", "trigger_decided"], block)
        # what the two trigger figures measured, asserted: armed SEARCHING no call fires and the search stays SEARCHING; decided, only the arming call fired
        rp.enter(err8, MU)
        arm_trigger(False)
        for _ in range(5):
            rp.trigger(0, a_out)
        live, fs_live = rp.state(), fs.state()
        arm_trigger(True)
        for _ in range(5):
            rp.trigger(0, a_out)
        decided, fs_decided = rp.state(), fs.state()
        assert live["triggers_orig"] == 0 and fs_live["status_name"] == "searching", (live, fs_live)
        assert decided["triggers_orig"] == 1 and fs_decided["status_name"] == "failed", (decided, fs_decided)
        res["trigger_check"] = {"searching": {"fired": live["triggers_orig"], "alpha_min": live["alpha_min"], "alpha": fs_live["alpha"]},
                                "decided": {"fired": decided["triggers_orig"], "status": fs_decided["status_name"]}}
        res["state_after_the_calls"] = rp.state()
        u = {key: v["us_median"] for key, v in res["us_per_call"].items()}
        res["rmu_error_over_resto_error"] = u["rmu_error"] / u["resto_error"]

        # ---- the rule and its read-back, wall clock ----------------------------------------------------------------------------------
        def device_rule(words):
            rp.error(state, rd, cd, out=w32)
            rp.update(words if words is not None else w32)
            return rp.state()

        def host_rule(passes):
            for _ in range(passes):
                resto.error(state, rd, cd, mu, zeta, out=e8)
                BarrierLayer.optimality_error(e8, counts_r)
            return resto.state()

        def wall(fn, before):
            for _ in range(3):
                before()
                fn()
            meds = []
            for _ in range(repeats):
                total = 0.0
                for _ in range(block):
                    before()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    total += time.perf_counter() - t0
                meds.append(1e6 * total / block)
            return {"us_median": float(np.median(meds)), "us_min": min(meds), "us_max": max(meds)}
        reset = lambda: rp.inner_mu.reset(mu)
        s0, s2 = (reset(), device_rule(None))[1], (reset(), device_rule(w_two))[1]
        assert s2["decreases_last"] == 2 and s2["changed"], s2
        res["decreases"] = {"rule_0": s0["decreases_last"], "rule_2": s2["decreases_last"]}      # (rule_0: what the state's own words decide)
        res["wall_us"] = {"rule_0": wall(lambda: device_rule(None), reset), "host_rule_0": wall(lambda: host_rule(1), reset),
                          "rule_2": wall(lambda: device_rule(w_two), reset), "host_rule_2": wall(lambda: host_rule(3), reset)}
        res["host_rule_0_over_rule_0"] = res["wall_us"]["host_rule_0"]["us_median"] / res["wall_us"]["rule_0"]["us_median"]
        res["host_rule_2_over_rule_2"] = res["wall_us"]["host_rule_2"]["us_median"] / res["wall_us"]["rule_2"]["us_median"]

        # ---- one iteration: eager and unbound against bound and captured ---------------------------------------------------------------
        prepare()
        bind(True)
        iteration(True)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            gm._sync_stream()
            iteration(True)
        gm._sync_stream()
        calls["graph_bound"] = graph.replay
        calls["iteration_bound"] = lambda: iteration(True)
        arm["graph_bound"] = arm["iteration_bound"] = lambda: bind(True)
        res["us_per_iteration"] = timed(["iteration_unbound", "iteration_bound", "graph_bound"], max(2, block // 10))
        it = {key: v["us_median"] for key, v in res["us_per_iteration"].items()}
        res["iteration_unbound_over_graph_bound"] = it["iteration_unbound"] / it["graph_bound"]
        bind(False)
    gm.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=CASES)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--block", type=int, default=100, help="calls between one event pair (a tenth of it for the iterations)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per case (child process)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rmu.json"))
    a = ap.parse_args()
    if a.case:
        print(json.dumps(one(a.case, a.block, a.repeats)))
        return 0
    doc = {"what": "tools/rmu_bench.py: µs per call of iem_rmu_error beside iem_resto_error (with the algorithmic bytes), of iem_rmu_enter / _update / _trigger — device events "
                   "around blocks of back-to-back calls; wall-clock µs of the restoration rule with its read-back (rmu_error + rmu_update + rmu_state) against the host sequence "
                   "(resto.error + a read-back per pass + resto.state()) with no and with two decreases; µs per restoration iteration eager and unbound, eager and bound, and "
                   "bound as one captured graph; warm, the calls taking turns; median / min / max over the blocks; reports, sets no threshold",
           "cases": []}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for case in a.cases.split(","):
        r = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--case", case, "--block", str(a.block),
                            "--repeats", str(a.repeats)], stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            print(f"{case}: FAILED with exit status {r.returncode}; nothing more is started", file=sys.stderr)
            return 1
        doc["cases"].append(json.loads(r.stdout.strip().splitlines()[-1]))
        c = doc["cases"][-1]
        print(case, {q: round(v["us_median"], 2) for q, v in {**c["us_per_call"], **c["wall_us"], **c["us_per_iteration"]}.items()}, "us", flush=True)
        with open(a.out, "w") as f:      # after every case: what was measured stays if a later case fails
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
