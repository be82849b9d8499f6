#!/usr/bin/env python3
"""What the starting point on the device (iem_init_*) costs per call, measured in one process per case.

  ls_terms                        iem_init_ls_terms: sigma, dcon and the right-hand side of the least-squares estimate
  ls_apply                        iem_init_ls_apply with an estimate that is accepted (the seed copy, the norm, the apply) — and
  ls_apply_rejected               with y_max = 0 and on_reject = 1: the seed copy and the norm, then an apply that stores four words
  warm, barrier_start             iem_init_warm beside iem_barrier_start on the same point: the same primal push, but the multipliers
                                  are read and clamped where barrier_start writes 1.0, and y is read and written
  init_mu, mu_reset               iem_init_mu (one workgroup, the twelve words in, seven words of the iem_mu block out) beside
                                  iem_mu_reset
  mu_error                        the call that feeds iem_init_mu

The sizes and the method of tools/mpc_bench.py: per case one child process under its own `timeout` (the parent never opens the GPU and
stops at the first child that fails); every call warmed, then blocks of back-to-back calls between ONE event pair, `--repeats` blocks
each, the calls taking turns; median, minimum and maximum per call over the blocks, with the algorithmic bytes.  No duration existed
before this tool: it reports and sets no threshold.

  python tools/init_bench.py --out profiles/init.json
  python tools/init_bench.py --case opf_10000          (one case, JSON on stdout)
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
MU, RELAX, PUSH, FRAC = 0.1, 1e-8, 1e-2, 1e-2


def one(case, block, repeats):
    import numpy as np
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib, transcribe, workloads
    from infiniteexamodels.jl_amd.barrier import BarrierLayer, BarrierParameter, StartingPoint
    from infiniteexamodels.jl_amd.model import ExaModel
    gm = ExaModel(transcribe.exa_core(eval(MODELS[case], {"workloads": workloads})), device=0)
    meta = gm.meta
    n, m = int(meta.nvar), int(meta.ncon)
    lvar, uvar, lcon, ucon = (np.asarray(a, dtype=np.float64) for a in (meta.lvar, meta.uvar, meta.lcon, meta.ucon))
    parts, fx, fc, info = iemlib.barrier_analyse(lvar, uvar, lcon, ucon, RELAX)
    rng = np.random.default_rng(0)
    hasL, hasU, gL, gU = (fx & 1) > 0, (fx & 2) > 0, (fc & 1) > 0, (fc & 2) > 0
    T = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")
    new = lambda k: torch.empty(k, dtype=torch.float64, device="cuda")
    xd, yd = T(np.asarray(meta.x0, dtype=np.float64) + 0.1 * rng.standard_normal(n)), T(0.1 * rng.standard_normal(m))
    _, cd, rd = gm.eval_residual(xd, yd)
    mult = lambda k: T(10.0 ** rng.uniform(-2, 2, k))
    state = (xd, cd.clone(), yd, mult(n), mult(n), mult(m), mult(m))
    nz, mi = info["nz"], info["n_ineq"]
    with_x = int((hasL | hasU).sum())
    # algorithmic bytes, counted as for the sibling kernels: flags, then 8-byte words per entry and per present bound
    nL, nU, mL, mU = int(hasL.sum()), int(hasU.sum()), int(gL.sum()), int(gU.sum())
    b_terms = (n + m) + 8 * (n + nL + nU + mi + mL + mU) + 8 * (n + m + n + m)      # flags; r, z*, y, v* read; sigma, dcon, rhs written
    b_apply = 8 * (2 * m + 3 * m)                                        # the norm reads y and delta, the apply reads them again and writes y
    b_norm = 8 * 2 * m
    b_start = (n + m) + 8 * (2 * with_x + nL + nU + 2 * n + mi + mL + mU + 3 * mi)      # flags; x in place, its bounds, zL, zU written; c, the rows' bounds, s, vL, vU written
    b_warm = (n + m) + 8 * (2 * with_x + nL + nU + 2 * n + 2 * m + 2 * mi + mL + mU + 2 * mi + nz)      # ... and y and s in place, the nz present multipliers read
    res = {"case": case, "model": MODELS[case], "device": torch.cuda.get_device_name(0), "repeats": repeats, "calls_per_block": block, **info,
           "bytes": {"ls_terms": b_terms, "ls_apply": b_apply, "ls_apply_rejected": b_norm, "barrier_start": b_start, "warm": b_warm}}

    with BarrierLayer(gm, relax=RELAX) as bar, BarrierParameter(bar, mu_init=MU) as par, StartingPoint(bar, warm_push=PUSH, warm_frac=FRAC, y_max=1e300) as init, \
            StartingPoint(bar, y_max=0.0, on_reject=1) as never:
        sigma, dcon, rhs, w = new(n), new(m), new(n + m), new(12)
        sol = torch.zeros(n + m, dtype=torch.float64, device="cuda")      # delta = 0: y stays where it is, call after call
        start_out = (new(m), new(n), new(n), new(m), new(m))
        par.error(state, rd, cd, out=w)
        calls = {"ls_terms": lambda: init.ls_terms(state, rd, out=(sigma, dcon, rhs)), "ls_apply": lambda: init.ls_apply(sol, yd),
                 "ls_apply_rejected": lambda: never.ls_apply(sol, yd), "warm": lambda: init.warm(state),
                 "barrier_start": lambda: bar.start(xd, cd, y=yd, bound_push=PUSH, bound_frac=FRAC, out=start_out), "mu_error": lambda: par.error(state, rd, cd, out=w),
                 "init_mu": lambda: init.mu(w, par), "mu_reset": lambda: par.reset(MU)}

        def timed(names, blk):
            for nm in names:
                for _ in range(3):
                    calls[nm]()
            torch.cuda.synchronize()
            us = {nm: [] for nm in names}
            for _ in range(repeats):
                for nm in names:
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(blk):
                        calls[nm]()
                    e1.record(); torch.cuda.synchronize()
                    us[nm].append(1e3 * e0.elapsed_time(e1) / blk)
            return {nm: {"us_median": float(np.median(v)), "us_min": min(v), "us_max": max(v)} for nm, v in us.items()}
        res["us_per_call"] = timed(list(calls), block)
        u = {key: v["us_median"] for key, v in res["us_per_call"].items()}
        res["warm_over_barrier_start"] = u["warm"] / u["barrier_start"]
        res["init_mu_over_mu_reset"] = u["init_mu"] / u["mu_reset"]
        res["state"] = {"accepting": init.state(), "rejecting": never.state()}
        assert res["state"]["accepting"]["accepted"] and (not res["state"]["rejecting"]["accepted"] or m == 0), res["state"]
    gm.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=CASES)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--block", type=int, default=100, help="calls between one event pair")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per case (child process)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "init.json"))
    a = ap.parse_args()
    if a.case:
        print(json.dumps(one(a.case, a.block, a.repeats)))
        return 0
    doc = {"what": "tools/init_bench.py: µs per call of iem_init_ls_terms, iem_init_ls_apply (accepted; and rejected with y kept), iem_init_warm beside iem_barrier_start on the "
                   "same point, iem_init_mu beside iem_mu_reset, and iem_mu_error — device events around blocks of back-to-back calls — with the algorithmic bytes; warm, "
                   "the calls taking turns; median / min / max over the blocks; reports, sets no threshold",
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
        print(case, {q: round(v["us_median"], 2) for q, v in c["us_per_call"].items()}, "us", flush=True)
        with open(a.out, "w") as f:      # after every case: what was measured stays if a later case fails
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
