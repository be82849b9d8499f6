#!/usr/bin/env python3
"""What the stopping test and the kept iterate on the device (iem_conv_*) cost per call, measured in one process per case.

  check                           iem_conv_check: the seed copy, max |x| over the variables, the decision (one workgroup)
  step                            iem_conv_step: the seed copy, the two maxima over x, s, sol, ds, the decision
  keep_0, keep_1                  iem_conv_keep with the word keep at 0 (every thread reads one word and returns) and at 1 (the copy)
  restore                         iem_conv_restore with a point held
  torch_copy                      beside keep_1: torch `copy_` of the same seven vectors into seven tensors (seven launches, every entry)
  mu_error                        beside check and step: the call that feeds the check

The sizes and the method of tools/init_bench.py: per case one child process under its own `timeout` (the parent never opens the GPU
and stops at the first child that fails); every call warmed, then blocks of back-to-back calls between ONE event pair, `--repeats`
blocks each, the calls taking turns; median, minimum and maximum per call over the blocks, with the algorithmic bytes.  No duration
existed for these calls before this tool: it reports and sets no threshold.  These launches sit near the launch floor, so the ratios
follow the bytes only at the largest size.

  python tools/conv_bench.py --out profiles/conv.json
  python tools/conv_bench.py --case opf_10000          (one case, JSON on stdout)
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
MU, RELAX = 0.1, 1e-8


def one(case, block, repeats):
    import numpy as np
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib, transcribe, workloads
    from infiniteexamodels.jl_amd.barrier import BarrierLayer, BarrierParameter, ConvergenceCheck
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
    mi = info["n_ineq"]
    nL, nU, mL, mU = int(hasL.sum()), int(hasU.sum()), int(gL.sum()), int(gU.sum())
    # algorithmic bytes, counted as for the sibling kernels: flags, then 8-byte words per entry read or written
    b_check = 8 * n                                                     # x read (the decision: a few words)
    b_step = m + 8 * (2 * n + m + 2 * mi)                               # the rows' flags; x and dx, dy, s and ds of inequality rows read
    b_keep1 = (n + m) + 8 * (n + nL + nU + m + mi + mL + mU) + 8 * (3 * n + m + 3 * mi)      # flags; the state read; every kept entry written
    b_restore = (n + m) + 2 * 8 * (n + nL + nU + m + mi + mL + mU)      # flags; the entries keep reads, read and written
    b_copy = 2 * 8 * (3 * n + 4 * m)                                    # torch: every entry of the seven vectors read and written
    res = {"case": case, "model": MODELS[case], "device": torch.cuda.get_device_name(0), "repeats": repeats, "calls_per_block": block, **info,
           "bytes": {"check": b_check, "step": b_step, "keep_0": 8, "keep_1": b_keep1, "restore": b_restore, "torch_copy": b_copy}}

    far = dict(acceptable_iter=0, max_iter=2 ** 40)      # never latches: the calls below repeat the same work, call after call
    with BarrierLayer(gm, relax=RELAX) as bar, BarrierParameter(bar, mu_init=MU) as par, ConvergenceCheck(par, **far) as conv, ConvergenceCheck(par, **far) as idle, \
            ConvergenceCheck(par, **far) as holding:
        w, f = new(12), T(np.array([1.0]))
        sol = T(0.1 * rng.standard_normal(n + m))
        ds = T(0.1 * rng.standard_normal(m))
        par.error(state, rd, cd, out=w)
        acceptable = torch.zeros(12, dtype=torch.float64, device="cuda")
        acceptable[0] = acceptable[2] = acceptable[3] = 1e-7
        holding.check(acceptable, f, xd)      # keep = 1 and, behind the first keep, a point held
        iterating = torch.zeros(12, dtype=torch.float64, device="cuda")      # E(0) = 1: the check goes through every branch and stays at ITERATING, whatever the point
        iterating[0] = 1.0
        holding.keep(state)
        into, targets = tuple(t.clone() for t in state), tuple(torch.empty_like(t) for t in state)

        def torch_copy():
            for dst, src in zip(targets, state):
                dst.copy_(src)

        calls = {"check": lambda: conv.check(iterating, f, xd), "step": lambda: conv.step(state, sol, ds), "keep_0": lambda: idle.keep(state), "keep_1": lambda: holding.keep(state),
                 "restore": lambda: holding.restore(into), "torch_copy": torch_copy, "mu_error": lambda: par.error(state, rd, cd, out=w)}

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
        res["keep_1_over_torch_copy"] = u["keep_1"] / u["torch_copy"]
        res["check_over_mu_error"] = u["check"] / u["mu_error"]
        res["step_over_mu_error"] = u["step"] / u["mu_error"]
        res["state"] = {"checking": conv.state(), "idle": idle.state(), "holding": holding.state()}
        s = res["state"]
        assert s["checking"]["status"] == 0 and not s["idle"]["keep"] and not s["idle"]["kept"] and s["holding"]["keep"] and s["holding"]["kept"], s
        assert all(torch.equal(a, b) for a, b in zip(into[:1], state[:1]))      # restore handed x back
    gm.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=CASES)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--block", type=int, default=100, help="calls between one event pair")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per case (child process)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv.json"))
    a = ap.parse_args()
    if a.case:
        print(json.dumps(one(a.case, a.block, a.repeats)))
        return 0
    doc = {"what": "tools/conv_bench.py: µs per call of iem_conv_check, iem_conv_step, iem_conv_keep with the word at 0 and at 1, iem_conv_restore, beside iem_mu_error and "
                   "torch copy_ of the same seven vectors — device events around blocks of back-to-back calls — with the algorithmic bytes; warm, the calls taking turns; "
                   "median / min / max over the blocks; reports, sets no threshold",
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
