#!/usr/bin/env python3
"""What the barrier parameter on the device (iem_mu_*) costs per call, and what "stopping test + mu rule" costs per iteration, against
the host's way of tests/search_loop.py (lines 37–49), measured in the same process.

  barrier_error, mu_error                         µs per call on the same state: they read the same bytes, mu_error reduces three more
                                                  values (the minimum, the sum and the count of the products); the ratio is reported,
                                                  there is no gate
  mu_update                                       µs per call (one workgroup; words that leave mu alone)
  rule_k0, rule_k2                                ONE iem_mu_error + iem_mu_update + iem_mu_state (the one read-back), with options under
                                                  which the update decreases mu k = 0 / k = 2 times; rule_k2 also holds the
                                                  iem_mu_reset that puts mu back for the next repetition
  host_k0, host_k2                                iem_barrier_error(0) + read, k × (iem_barrier_error(mu) + read), iem_barrier_error(mu):
                                                  the sequence of tests/search_loop.py, every read a .tolist() and
                                                  BarrierLayer.optimality_error

The sizes and the method of tools/barrier_bench.py and tools/search_bench.py: per case one child process under its own `timeout` (the
parent never opens the GPU and stops at the first child that fails); every sequence warmed, then blocks of back-to-back calls between
ONE event pair (the sequences with a read-back: wall clock around the block), `--repeats` blocks each, the sequences taking turns;
median, minimum and maximum per call over the blocks.

  python tools/mu_bench.py --out profiles/mu.json
  python tools/mu_bench.py --case opf_10000          (one case, JSON on stdout)
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ("pandemic_110_128", "opf_10000", "quadrotor_16000", "quadrotor_100000")
MODELS = {"pandemic_110_128": "workloads.pandemic(110, 128)", "opf_10000": "workloads.opf(10000)", "quadrotor_16000": "workloads.quadrotor(16000)",
          "quadrotor_100000": "workloads.quadrotor(100000)"}
MU, RELAX = 0.1, 1e-8
# kappa_eps decides whether the barrier problem counts as solved: never (k = 0), or always, down to a floor that two decreases reach
RULE = {0: dict(kappa_eps=1e-300), 2: dict(kappa_eps=1e300, mu_floor=3e-3)}


def one(case, block, repeats):
    import numpy as np
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib, transcribe, workloads
    from infiniteexamodels.jl_amd.barrier import BarrierLayer, BarrierParameter
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
    xd, yd = T(x), T(0.1 * rng.standard_normal(m))
    _, cd, rd = gm.eval_residual(xd, yd)
    s = inside(cd.cpu().numpy(), parts["rl"], parts["ru"], gL, gU)
    mult = lambda k: T(10.0 ** rng.uniform(-2, 2, k))
    state = (xd, T(s), yd, mult(n), mult(n), mult(m), mult(m))
    res = {"case": case, "model": MODELS[case], "device": torch.cuda.get_device_name(0), "repeats": repeats, "calls_per_block": block, **info}

    with BarrierLayer(gm, relax=RELAX) as bar, BarrierParameter(bar, mu_init=MU, kappa_eps=1e-300) as par:
        counts = (info["ncon"], info["nz"])
        e8, w12 = gm._new(8), gm._new(12)
        rules = {k: BarrierParameter(bar, mu_init=MU, **o) for k, o in RULE.items()}
        par.error(state, rd, cd, out=w12)
        bar.error(state, rd, cd, 0.0, out=e8)
        torch.cuda.synchronize()
        assert torch.equal(w12[:8].view(torch.int64), e8.view(torch.int64)), "words 0-7 are not iem_barrier_error's"

        def rule(k):
            p = rules[k]
            if k:
                p.reset(MU)      # re-arms the measurement: mu back at its start (an iteration of a solver has no such call)
            p.error(state, rd, cd, out=w12)
            p.update(w12)
            return p.state()

        def host(k):
            mu = MU
            BarrierLayer.optimality_error(bar.error(state, rd, cd, 0.0, out=e8), counts)
            for _ in range(k):
                BarrierLayer.optimality_error(bar.error(state, rd, cd, mu, out=e8), counts)
                mu = max(1e-11, min(0.2 * mu, mu ** 1.5))
            bar.error(state, rd, cd, mu, out=e8)
        for k in RULE:
            st = rule(k)
            assert st["decreases"] == k and st["status_name"] == "iterating", (k, st)
        calls = {"barrier_error": lambda: bar.error(state, rd, cd, 0.0, out=e8), "mu_error": lambda: par.error(state, rd, cd, out=w12), "mu_update": lambda: par.update(w12),
                 "rule_k0": lambda: rule(0), "rule_k2": lambda: rule(2), "host_k0": lambda: host(0), "host_k2": lambda: host(2)}

        def timed(names, blk, wall):
            for nm in names:
                for _ in range(3):
                    calls[nm]()
            torch.cuda.synchronize()
            us = {nm: [] for nm in names}
            for _ in range(repeats):
                for nm in names:
                    torch.cuda.synchronize()
                    if wall:
                        t0 = time.perf_counter()
                        for _ in range(blk):
                            calls[nm]()
                        torch.cuda.synchronize()
                        us[nm].append(1e6 * (time.perf_counter() - t0) / blk)
                    else:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(blk):
                            calls[nm]()
                        e1.record(); torch.cuda.synchronize()
                        us[nm].append(1e3 * e0.elapsed_time(e1) / blk)
            return {nm: {"us_median": float(np.median(v)), "us_min": min(v), "us_max": max(v)} for nm, v in us.items()}
        res["us_per_call"] = timed(["barrier_error", "mu_error", "mu_update"], block, wall=False)
        res["mu_error_over_barrier_error"] = res["us_per_call"]["mu_error"]["us_median"] / res["us_per_call"]["barrier_error"]["us_median"]
        res["us_per_iteration_wall_clock"] = timed(["rule_k0", "host_k0", "rule_k2", "host_k2"], max(2, block // 2), wall=True)
        w = res["us_per_iteration_wall_clock"]
        res["host_over_rule"] = {k: w[f"host_{k}"]["us_median"] / w[f"rule_{k}"]["us_median"] for k in ("k0", "k2")}
        for p in rules.values():
            p.close()
    gm.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=CASES)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--block", type=int, default=100, help="calls between one event pair (half of it for the sequences with a read-back)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per case (child process)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mu.json"))
    a = ap.parse_args()
    if a.case:
        print(json.dumps(one(a.case, a.block, a.repeats)))
        return 0
    doc = {"what": "tools/mu_bench.py: µs per call of iem_barrier_error, iem_mu_error (same bytes, three more reduced values) and iem_mu_update — device events "
                   "around blocks of back-to-back calls — and µs per 'stopping test + mu rule' — wall clock around blocks, every sequence ends in a read-back: "
                   "error + update + iem_mu_state (k = 2: and the iem_mu_reset that re-arms it) against error(0) + read, k × (error(mu) + read), error(mu) as tests/search_loop.py has it, for "
                   "k = 0 and k = 2 decreases; warm, the sequences taking turns; median / min / max over the blocks",
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
        print(case, {q: round(v["us_median"], 2) for q, v in {**c["us_per_call"], **c["us_per_iteration_wall_clock"]}.items()}, "us", flush=True)
        with open(a.out, "w") as f:      # after every case: what was measured stays if a later case fails
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
