#!/usr/bin/env python3
"""What the filter line search on the device (iem_search_*) costs per call and per rung, against the same rung done the host's way —
the torch expressions and `.item()` reads of contrib/ipm.py's line search (kept here as the baseline, measured in the same process).

  begin, trial, accept, accept_decided            µs per call (accept: the whole test on an empty filter, rejecting; accept_decided: a
                                                  search that has its answer — the call returns at its first test)
  rung                                            trial + iem_obj_device + iem_cons + iem_barrier_merit + accept, eager
  ladder4_graph                                   begin + four rungs captured once and replayed: µs per replay (per rung: a quarter)
  host_rung                                       the same rung the host's way: two torch launches for the trial point, iem_obj (a
                                                  synchronous read), iem_cons, theta and sum log gap by torch with two .item() reads,
                                                  the filter test in Python
  host_slope                                      the slope by two dot products and two .item() reads, against `begin`

The state is strictly interior, the direction is N(0, 1)·1e-5 so that every trial point stays interior.  The search object of the
timings has max_trials = 2^62 and alpha_floor = 0: it never fails, so `accept` runs its whole test in every call of a block.  Per case
one child process under its own `timeout` (the parent never opens the GPU and stops at the first child that fails).  Every sequence
warmed, then blocks of back-to-back calls between ONE event pair, `--repeats` blocks each, the sequences taking turns; median, minimum
and maximum per call over the blocks.  Algorithmic bytes per call (counted from the sizes) are reported beside them.

  python tools/search_bench.py --out profiles/search.json
  python tools/search_bench.py --case opf_10000          (one case, JSON on stdout)
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
MU, TAU, RELAX = 0.1, 0.99, 1e-8


def alg_bytes(info):
    """bytes every call has to move, from the sizes alone: doubles read + written, the bounds and the flag bytes included"""
    n, m, mi = info["nvar"], info["ncon"], info["n_ineq"]
    return {"begin": (3 * n + 2 * mi) * 8 + 2 * n * 8 + n + 2 * mi * 8 + m + 11 * 8 + 16 * 8,      # x, g, dx, s, ds; xl, xu, fx, rl, ru, fc; scalars; the block
            "trial": (2 * n + 2 * mi) * 8 + m + 16 + (n + mi) * 8,                                   # x, dx, s, ds, fc, two words of the block; xt, st
            "accept": 16 * 8 + 3 * 8 + 9 * 8}                                                        # the block, ft and the two sums; what it writes (+ 16 bytes per filter entry)


def one(case, block, repeats):
    import numpy as np
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib, transcribe, workloads
    from infiniteexamodels.jl_amd.barrier import BarrierLayer, FilterSearch
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
    res = {"case": case, "model": MODELS[case], "device": torch.cuda.get_device_name(0), "repeats": repeats, "calls_per_block": block, **info}

    with BarrierLayer(gm, relax=RELAX) as bar, FilterSearch(bar, max_trials=2 ** 62, alpha_floor=0.0) as fs, FilterSearch(bar) as done:
        err = bar.error(state, rd, cd, MU)
        alpha0 = T([1.0, 1.0])
        alpha = alpha0.clone()
        xt, st, ct, ft, mt = gm._new(n), torch.zeros(m, dtype=torch.float64, device="cuda"), gm._new(m), gm._new(1), gm._new(2)
        far = T([1e300, 0.0])      # a theta above theta_max: every accept rejects, after its whole test
        # `done`: a search that has accepted (theta_t = 0 on an empty filter is an h-type or an f-type step)
        done.begin(state, gd, sol, ds, f0, err, alpha0, MU)
        done.accept(f0, T([0.0, float(err[7])]), MU, alpha0.clone())
        assert done.state()["status"] in (1, 2), done.state()

        def begin():
            alpha.copy_(alpha0)
            fs.begin(state, gd, sol, ds, f0, err, alpha, MU)

        def rung():
            fs.trial(state, sol, ds, xt, st)
            gm.obj_device(xt, out=ft)
            gm.cons(xt, ct)
            bar.merit(xt, st, ct, out=mt)
            fs.accept(ft, mt, MU, alpha)

        def ladder():
            begin()
            for _ in range(4):
                rung()
        calls = {"begin": lambda: fs.begin(state, gd, sol, ds, f0, err, alpha0, MU), "trial": lambda: fs.trial(state, sol, ds, xt, st),
                 "accept": lambda: fs.accept(ft, far, MU, alpha), "accept_decided": lambda: done.accept(ft, far, MU, alpha), "rung": rung}
        begin()
        ladder()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ladder()
        gm._sync_stream()
        calls["ladder4_graph"] = g.replay

        # ---- the baseline: contrib/ipm.py's line search on compacted inequality rows ------------------------------------
        xl, xu = T(parts["xl"]), T(parts["xu"])
        ine_idx = torch.as_tensor(np.nonzero(~eq)[0], device="cuda")
        sl, su = T(parts["rl"][~eq]), T(parts["ru"][~eq])
        Lx, Ux, Ls, Us = torch.isfinite(xl), torch.isfinite(xu), torch.isfinite(sl), torch.isfinite(su)
        ceq = T(parts["ceq"])
        big, bigs = torch.full_like(xl, float("inf")), torch.full_like(sl, float("inf"))
        Z = lambda on, v: torch.where(on, v, torch.zeros_like(v))
        sc, dsc, dx = state[1][ine_idx], ds[ine_idx], sol[:n]
        hs = dict(step=1.0, filt=[], phi_f=0.0, viol=1.0, slope_b=-1.0, theta_ref=1.0)

        def host_rung():
            step = hs["step"]
            xt_, st_ = xd + step * dx, sc + step * dsc
            ft_ = gm.obj(xt_)
            gm.cons(xt_, ct)
            r = ct - ceq
            r[ine_idx] = ct[ine_idx] - st_
            vt = float(r.abs().sum().item())
            dL, dU, eL, eU = torch.where(Lx, xt_ - xl, big), torch.where(Ux, xu - xt_, big), torch.where(Ls, st_ - sl, bigs), torch.where(Us, su - st_, bigs)
            phibt = ft_ - MU * float((torch.log(dL[Lx]).sum() + torch.log(dU[Ux]).sum() + torch.log(eL[Ls]).sum() + torch.log(eU[Us]).sum()).item())
            ok = np.isfinite(phibt) and vt <= 1e4 * hs["theta_ref"] and not any(vt >= th and phibt >= ph for th, ph in hs["filt"])
            ftype = hs["slope_b"] < 0.0 and hs["viol"] <= 1e-4 * hs["theta_ref"] and step * (-hs["slope_b"]) ** 2.3 > hs["viol"] ** 1.1
            if ok and ftype:
                accepted = phibt <= hs["phi_f"] + 1e-8 * step * hs["slope_b"] + 10.0 * np.finfo(float).eps * abs(hs["phi_f"])
            else:
                accepted = ok and (vt <= (1.0 - 1e-5) * hs["viol"] or phibt <= hs["phi_f"] - 1e-5 * hs["viol"])
            hs["step"] = 1.0 if accepted or step < 1e-3 else 0.5 * step
            return accepted

        def host_slope():
            dL, dU, eL, eU = torch.where(Lx, xd - xl, big), torch.where(Ux, xu - xd, big), torch.where(Ls, sc - sl, bigs), torch.where(Us, su - sc, bigs)
            gx = gd - Z(Lx, MU / dL) + Z(Ux, MU / dU)
            gs = -Z(Ls, MU / eL) + Z(Us, MU / eU)
            return float((gx @ dx).item()) + (float((gs @ dsc).item()) if dsc.numel() else 0.0)
        calls["host_rung"] = host_rung
        calls["host_slope"] = host_slope

        def timed(names, blk):
            for nm in names:
                begin()
                for _ in range(3):
                    calls[nm]()
            torch.cuda.synchronize()
            us = {nm: [] for nm in names}
            for _ in range(repeats):
                for nm in names:
                    begin()
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(blk):
                        calls[nm]()
                    e1.record(); torch.cuda.synchronize()
                    us[nm].append(1e3 * e0.elapsed_time(e1) / blk)
            return {nm: {"us_median": float(np.median(v)), "us_min": min(v), "us_max": max(v)} for nm, v in us.items()}
        res["us_per_call"] = timed(["begin", "trial", "accept", "accept_decided", "host_slope"], block)
        res["us_per_rung"] = timed(["rung", "ladder4_graph", "host_rung"], max(2, block // 10))
        res["us_per_rung"]["ladder4_graph"]["rungs_per_replay"] = 4
        res["alg_bytes_per_call"] = alg_bytes(info)
        final = fs.state()
        res["search_state_at_the_end"] = {k: final[k] for k in ("status_name", "trials", "filter_count", "slope")}
        res["slope_the_host_way"] = host_slope()      # (the two ways compute the same number, up to the summation order)
    gm.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=CASES)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--block", type=int, default=100, help="calls between one event pair (a tenth of it for the rungs)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per case (child process)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search.json"))
    a = ap.parse_args()
    if a.case:
        print(json.dumps(one(a.case, a.block, a.repeats)))
        return 0
    doc = {"what": "tools/search_bench.py: µs per call of iem_search_begin / _trial / _accept, µs per rung (trial + obj + cons + merit + accept) eager and as a "
                   "captured ladder of begin + four rungs, and the same rung and slope by the torch expressions and .item() reads of contrib/ipm.py's line "
                   "search; device events around blocks of back-to-back calls, warm, the sequences taking turns; median / min / max over the blocks; "
                   "algorithmic bytes counted from the sizes",
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
        print(case, {q: round(v["us_median"], 2) for q, v in {**c["us_per_call"], **c["us_per_rung"]}.items()}, "us", flush=True)
        with open(a.out, "w") as f:      # after every case: what was measured stays if a later case fails
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
