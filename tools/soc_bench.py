#!/usr/bin/env python3
"""What the second-order correction of the filter line search (iem_soc_*) costs per call, per round and per captured ladder, against
the same round done the host's way — torch expressions for csoc, rhs_soc and the trial point, `.item()` reads and the test in Python
(measured in the same process; the solve and the barrier step are the same device calls on both sides).

  open, rhs, trial, select                        µs per call; the block is set ACTIVE (select: ACCEPTED) once in front of a block of
                                                  calls — these four do not change it
  accept                                          µs per call, the whole test (rejecting: theta above theta_max): `restore` — a 128-byte
                                                  device-to-device copy that sets the block ACTIVE again — runs in front of every call and
                                                  is INCLUDED; `restore` alone is reported beside it
  accept_decided                                  a block that is not ACTIVE: the call returns at its first test
  round                                           restore + rhs + iem_kkt_solve_refined_diag + iem_barrier_step + trial + iem_obj_device +
                                                  iem_cons + iem_barrier_merit + accept, eager
  ladder_graph                                    begin; rung; open; 2 × round; select; 2 × rung captured once and replayed: µs per
                                                  replay (the state words it ends with are reported: they say which rounds were live)
  host_round                                      the same round the host's way

The state is strictly interior, the direction is N(0, 1)·1e-5 so that every trial point stays interior; the KKT object holds the
factors of the state's own matrix (delta_w = 1e-2, delta_c = 1e-6).  Per case one child process under its own `timeout` (the parent
never opens the GPU and stops at the first child that fails).  Every sequence warmed, then blocks of back-to-back calls between ONE
event pair, `--repeats` blocks each, the sequences taking turns; median, minimum and maximum per call over the blocks.  Algorithmic
bytes per call (counted from the sizes) are reported beside them.

  python tools/soc_bench.py --out profiles/soc.json
  python tools/soc_bench.py --case opf_10000          (one case, JSON on stdout)
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ("pandemic_110_128", "opf_10000", "quadrotor_16000", "quadrotor_100000")
MODELS = {"pandemic_110_128": "workloads.pandemic(110, 128)", "opf_10000": "workloads.opf(10000)", "quadrotor_16000": "workloads.quadrotor(16000)",
          "quadrotor_100000": "workloads.quadrotor(100000)"}
MU, TAU, RELAX, DW, DC = 0.1, 0.99, 1e-8, 1e-2, 1e-6


def alg_bytes(info):
    """bytes every call has to move, from the sizes alone (present bounds counted as if every inequality row had both)"""
    n, m, mi = info["nvar"], info["ncon"], info["n_ineq"]
    me = m - mi
    return {"open": 5 * 8 + 3 * 8,
            "rhs": n * 8 + me * 3 * 8 + mi * 9 * 8 + m + 3 * 8 + (n + 2 * m) * 8,      # rhs; c | csoc, ct, ceq; c | csoc, ct, st, s, y, rl, ru, vL, vU; fc; the block; rhs_soc, csoc
            "trial": (2 * n + 2 * mi) * 8 + m + 16 + (n + mi) * 8,                   # x, dx, s, ds, fc, a word of the block and alpha_soc[0]; xt, st
            "accept": 16 * 8 + 5 * 8 + 11 * 8,                                       # the block, ft, the two sums, alpha_soc; what it writes (+ 16 bytes per filter entry)
            "select": 8 + 2 * (3 * n + m + 3 * mi) * 8 + m}                          # a word; iff accepted: sol, dzL, dzU, ds, dvL, dvU read and written, fc


def one(case, block, repeats):
    import ctypes as C
    import numpy as np
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib, transcribe, workloads
    from infiniteexamodels.jl_amd.barrier import BarrierLayer, FilterSearch, SecondOrderCorrection
    from infiniteexamodels.jl_amd.kkt_chain import KKTObject
    from infiniteexamodels.jl_amd.model import ExaModel
    gm = ExaModel(transcribe.exa_core(eval(MODELS[case], {"workloads": workloads})), device=0)
    meta = gm.meta
    n, m = int(meta.nvar), int(meta.ncon)
    lvar, uvar, lcon, ucon = (np.asarray(a, dtype=np.float64) for a in (meta.lvar, meta.uvar, meta.lcon, meta.ucon))
    parts, fx, fc, info = iemlib.barrier_analyse(lvar, uvar, lcon, ucon, RELAX)
    rng = np.random.default_rng(0)
    hasL, hasU, gL, gU, eq = (fx & 1) > 0, (fx & 2) > 0, (fc & 1) > 0, (fc & 2) > 0, (fc & 4) > 0

    def inside(v, lo, hi, a, b):
        with np.errstate(invalid="ignore"):
            v = np.where(a & b, lo + rng.uniform(0.05, 0.95, len(v)) * (hi - lo), v)
            v = np.where(a & ~b, lo + 10.0 ** rng.uniform(-2, 1, len(v)), v)
            return np.where(b & ~a, hi - 10.0 ** rng.uniform(-2, 1, len(v)), v)
    x = inside(np.asarray(meta.x0, dtype=np.float64) + 0.1 * rng.standard_normal(n), parts["xl"], parts["xu"], hasL, hasU)
    T = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")
    xd, yd = T(x), T(0.1 * rng.standard_normal(m))
    f0, cd, rd = gm.eval_residual(xd, yd)
    gd = gm.grad(xd)
    s = inside(cd.cpu().numpy(), parts["rl"], parts["ru"], gL, gU)
    mult = lambda k: T(10.0 ** rng.uniform(-2, 2, k))
    state = (xd, T(s), yd, mult(n), mult(n), mult(m), mult(m))
    sol, ds = T(1e-5 * rng.standard_normal(n + m)), T(1e-5 * rng.standard_normal(m))
    new = lambda k: torch.empty(k, dtype=torch.float64, device="cuda")
    res = {"case": case, "model": MODELS[case], "device": torch.cuda.get_device_name(0), "repeats": repeats, "calls_per_block": block, **info}

    with BarrierLayer(gm, relax=RELAX) as bar, KKTObject(gm) as kkt, FilterSearch(bar, max_trials=2 ** 62, alpha_floor=0.0) as fs, \
            SecondOrderCorrection(fs, max_soc=16, kappa_soc=1.0) as soc:
        err = bar.error(state, rd, cd, MU)
        sigma, dcon, rhs = bar.terms(state, rd, cd, MU)
        jv, hv = new(int(meta.nnzj)), new(int(meta.nnzh))
        gm.jac_hess_coord(xd, yd, jv, hv, obj_weight=1.0)
        kkt.set_border(1)      # a dense border stays on the device: the solve synchronises nowhere and can be captured
        kkt.assemble(hv, jv, sigma, DW, DC, dcon=dcon, at=(xd, yd, 1.0))
        res["inertia"] = list(kkt.factor())
        L, k = kkt._handle()
        p = lambda t: C.c_void_p(t.data_ptr())

        def solve(b, out):      # one column, one refinement step, buffers of the caller: no allocation
            kkt._handle()
            iemlib.check(L.iem_kkt_solve_refined_diag(k, p(xd), p(yd), 1.0, p(sigma), p(dcon), DW, DC, 1, p(b), n + m, p(out), n + m, 1, None))
        alpha0 = T([1.0, 1.0])
        alpha = alpha0.clone()
        dirs = (ds, new(n), new(n), torch.zeros(m, dtype=torch.float64, device="cuda"), torch.zeros(m, dtype=torch.float64, device="cuda"))
        xt, st, ct, ft, mt = new(n), torch.zeros(m, dtype=torch.float64, device="cuda"), new(m), new(1), new(2)
        rhs_soc, sol_soc, alpha_soc = torch.zeros(n + m, dtype=torch.float64, device="cuda"), torch.zeros(n + m, dtype=torch.float64, device="cuda"), T([1.0, 1.0])
        dirs_soc = tuple(torch.zeros(q, dtype=torch.float64, device="cuda") for q in (m, n, n, m, m))
        far = T([1e300, 0.0])      # a theta above theta_max: every accept rejects, after its whole test
        # the block of a search one rejected trial in, ACTIVE / ACCEPTED, kept on the device and copied over the object's block
        fs.begin(state, gd, sol, ds, f0, err, alpha0, MU)
        fs.trial(state, sol, ds, xt, st)
        gm.cons(xt, ct)
        fs.accept(f0, far, MU, alpha)
        ctl_ptr, _ = fs.device()
        torch.cuda.synchronize()
        host_block = np.zeros(16)
        rt = C.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))
        rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        rt.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        assert rt.hipMemcpy(host_block.ctypes.data, ctl_ptr, 128, 2) == 0
        assert host_block.view(np.int64)[9] == 0 and host_block.view(np.int64)[10] == 1, host_block
        host_block[7], host_block[8] = 1.0, 1e290      # the rejected trial's phi, theta: every later theta (1e300) is no improvement
        blocks = {}
        for name, word in (("active", 1), ("accepted", 2), ("closed", 3)):
            b = host_block.copy()
            b.view(np.int64)[13], b.view(np.int64)[14], b[15] = word, 0, 1.0
            blocks[name] = T(b)

        def restore(name="active"):
            gm._sync_stream()
            stream = torch.cuda.current_stream().cuda_stream
            assert rt.hipMemcpyAsync(ctl_ptr, blocks[name].data_ptr(), 128, 3, stream) == 0

        def soc_round():
            restore()
            soc.rhs(state, cd, ct, st, rhs, MU, out=rhs_soc)
            solve(rhs_soc, sol_soc)
            bar.step(state, sol_soc, MU, TAU, out=dirs_soc, alpha=alpha_soc)
            soc.trial(state, sol_soc, dirs_soc[0], alpha_soc, xt, st)
            gm.obj_device(xt, out=ft)
            gm.cons(xt, ct)
            bar.merit(xt, st, ct, out=mt)
            soc.accept(ft, mt, alpha_soc, MU, alpha)

        def rung():
            fs.trial(state, sol, dirs[0], xt, st)
            gm.obj_device(xt, out=ft)
            gm.cons(xt, ct)
            bar.merit(xt, st, ct, out=mt)
            fs.accept(ft, mt, MU, alpha)

        def graph_round():
            soc.rhs(state, cd, ct, st, rhs, MU, out=rhs_soc)
            solve(rhs_soc, sol_soc)
            bar.step(state, sol_soc, MU, TAU, out=dirs_soc, alpha=alpha_soc)
            soc.trial(state, sol_soc, dirs_soc[0], alpha_soc, xt, st)
            gm.obj_device(xt, out=ft)
            gm.cons(xt, ct)
            bar.merit(xt, st, ct, out=mt)
            soc.accept(ft, mt, alpha_soc, MU, alpha)

        def ladder():
            alpha.copy_(alpha0)
            fs.begin(state, gd, sol, dirs[0], f0, err, alpha, MU)
            rung()
            soc.open()
            graph_round(); graph_round()
            soc.select(sol_soc, dirs_soc, sol, dirs)
            rung(); rung()
        bar.step(state, sol, MU, TAU, out=(torch.zeros(m, dtype=torch.float64, device="cuda"),) + dirs[1:], alpha=alpha0.clone())      # dzL .. dvU of the first-order direction (ds stays the random one)
        sol_keep, dirs_keep = sol.clone(), tuple(d.clone() for d in dirs)

        def ladder_fresh():      # (an accepted correction overwrites sol and dirs: start every replay from the same direction)
            sol.copy_(sol_keep)
            for d, k_ in zip(dirs, dirs_keep):
                d.copy_(k_)
        calls = {"restore": restore, "open": soc.open, "rhs": lambda: soc.rhs(state, cd, ct, st, rhs, MU, out=rhs_soc),
                 "trial": lambda: soc.trial(state, sol_soc, dirs_soc[0], alpha_soc, xt, st),
                 "accept": lambda: (restore(), soc.accept(ft, far, alpha_soc, MU, alpha)),
                 "accept_decided": lambda: soc.accept(ft, far, alpha_soc, MU, alpha),
                 "select": lambda: soc.select(sol_soc, dirs_soc, sol, dirs), "round": soc_round}
        before = {"restore": "active", "open": "closed", "rhs": "active", "trial": "active", "accept": "active", "accept_decided": "closed", "select": "accepted",
                  "round": "active", "ladder_graph": "closed", "host_round": "closed"}
        soc_round()
        ladder_fresh(); ladder()
        torch.cuda.synchronize()
        res["soc_state_after_the_ladder"] = {q: soc.state()[q] for q in ("status", "state_name", "rounds")}
        g = torch.cuda.CUDAGraph()
        ladder_fresh()
        torch.cuda.synchronize()
        with torch.cuda.graph(g):
            ladder()
        gm._sync_stream()
        calls["ladder_graph"] = lambda: (ladder_fresh(), g.replay())

        # ---- the baseline: the same round by torch expressions, .item() reads and the test in Python ----------------------------------
        xl, xu = T(parts["xl"]), T(parts["xu"])
        ine = torch.as_tensor(~eq, device="cuda")
        rl, ru, ceq = T(np.where(np.isfinite(parts["rl"]), parts["rl"], 0.0)), T(np.where(np.isfinite(parts["ru"]), parts["ru"], 0.0)), T(parts["ceq"])
        Lx, Ux, Ls, Us = torch.isfinite(xl), torch.isfinite(xu), torch.as_tensor(gL, device="cuda"), torch.as_tensor(gU, device="cuda")
        zero_m = torch.zeros(m, dtype=torch.float64, device="cuda")
        hs = dict(alpha_prev=1.0, alpha_max=1.0, filt=[], phi0=0.0, theta0=1.0, slope=-1.0, theta_min=1e-4, theta_max=1e4, theta_prev=1.0, rounds=0)
        csoc_h = torch.where(ine, cd - state[1], cd - ceq)

        def host_round():
            s_, y_, vL_, vU_ = state[1], state[2], state[5], state[6]
            inf_t = torch.where(ine, ct - st, ct - ceq)
            csoc = hs["alpha_prev"] * csoc_h + inf_t
            eL, eU = s_ - rl, ru - s_
            sigs = torch.where(Ls, vL_ / eL, zero_m) + torch.where(Us, vU_ / eU, zero_m)
            rs = (torch.where(Us, MU / eU, zero_m) - torch.where(Ls, MU / eL, zero_m)) - y_
            rhs_soc[:n] = rhs[:n]
            rhs_soc[n:] = torch.where(ine, -(csoc + rs / sigs), -csoc)
            solve(rhs_soc, sol_soc)
            bar.step(state, sol_soc, MU, TAU, out=dirs_soc, alpha=alpha_soc)
            a_soc = float(alpha_soc[0].item())
            xt_ = xd + a_soc * sol_soc[:n]
            st_ = torch.where(ine, s_ + a_soc * dirs_soc[0], zero_m)
            ft_ = gm.obj(xt_)
            gm.cons(xt_, ct)
            theta_t = float(torch.where(ine, ct - st_, ct - ceq).abs().sum().item())
            logs = torch.log((xt_ - xl)[Lx]).sum() + torch.log((xu - xt_)[Ux]).sum() + torch.log((st_ - rl)[Ls]).sum() + torch.log((ru - st_)[Us]).sum()
            phi_t = ft_ - MU * float(logs.item())
            a = hs["alpha_max"]
            ok = np.isfinite(phi_t) and np.isfinite(theta_t) and theta_t <= hs["theta_max"] and not any(theta_t >= th and phi_t >= ph for th, ph in hs["filt"])
            switching = hs["slope"] < 0.0 and hs["theta0"] <= hs["theta_min"] and a * (-hs["slope"]) ** 2.3 > hs["theta0"] ** 1.1
            if ok and switching:
                accepted = phi_t <= hs["phi0"] + 1e-8 * a * hs["slope"] + 10.0 * np.finfo(float).eps * abs(hs["phi0"])
            else:
                accepted = ok and (theta_t <= (1.0 - 1e-5) * hs["theta0"] or phi_t <= hs["phi0"] - 1e-8 * hs["theta0"])
            go_on = not accepted and hs["rounds"] + 1 < 4 and np.isfinite(theta_t) and theta_t <= 0.99 * hs["theta_prev"]
            hs["alpha_prev"] = a_soc if go_on else 1.0
            return accepted
        calls["host_round"] = host_round

        def timed(names, blk):
            for nm in names:
                restore(before[nm])
                for _ in range(3):
                    calls[nm]()
            torch.cuda.synchronize()
            us = {nm: [] for nm in names}
            for _ in range(repeats):
                for nm in names:
                    restore(before[nm])
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(blk):
                        calls[nm]()
                    e1.record(); torch.cuda.synchronize()
                    us[nm].append(1e3 * e0.elapsed_time(e1) / blk)
            return {nm: {"us_median": float(np.median(v)), "us_min": min(v), "us_max": max(v)} for nm, v in us.items()}
        res["us_per_call"] = timed(["restore", "open", "rhs", "trial", "accept", "accept_decided", "select"], block)
        res["us_per_round"] = timed(["round", "ladder_graph", "host_round"], max(2, block // 10))
        res["us_per_round"]["ladder_graph"]["what"] = "begin; rung; open; 2 x round; select; 2 x rung, and the copies that restore sol and dirs in front of a replay"
        res["alg_bytes_per_call"] = alg_bytes(info)
    gm.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=CASES)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--block", type=int, default=100, help="calls between one event pair (a tenth of it for the rounds)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per case (child process)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "soc.json"))
    a = ap.parse_args()
    if a.case:
        print(json.dumps(one(a.case, a.block, a.repeats)))
        return 0
    doc = {"what": "tools/soc_bench.py: µs per call of iem_soc_open / _rhs / _trial / _accept / _select, µs per round (rhs + refined solve + barrier step + trial + obj + "
                   "cons + merit + accept) eager, µs per replay of the captured ladder begin; rung; open; 2 x round; select; 2 x rung, and the same round by torch "
                   "expressions, .item() reads and the test in Python; device events around blocks of back-to-back calls, warm, the sequences taking turns; median / "
                   "min / max over the blocks; algorithmic bytes counted from the sizes",
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
        print(case, {q: round(v["us_median"], 2) for q, v in {**c["us_per_call"], **c["us_per_round"]}.items()}, "us", flush=True)
        with open(a.out, "w") as f:      # after every case: what was measured stays if a later case fails
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
