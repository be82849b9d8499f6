#!/usr/bin/env python3
"""What the adaptive barrier parameter on the device (iem_amu_*) costs per call, and what "probe + rule + read-back" costs per
iteration against the same quantities by torch expressions, measured in the same process.

  mu_error, amu_probe                             µs per call on the same state: the probe reads six direction vectors more (and
                                                  neither y, r nor c), computes no logarithm and reduces two values where mu_error
                                                  reduces ten; the ratio and the algorithmic bytes of both are reported, there is no gate
  amu_update                                      µs per call (one workgroup)
  rule                                            ONE iem_amu_probe + iem_amu_update + iem_amu_state (the one read-back); the state does
                                                  not move between the calls, so once the ring of references is full the update
                                                  takes its fixed-mode branch
  torch                                           the probe's sum and NaN count by torch expressions over the full vectors (masks for
                                                  the present bounds), one read-back of both, sigma and mu on the host

The sizes and the method of tools/mu_bench.py: per case one child process under its own `timeout` (the parent never opens the GPU and
stops at the first child that fails); every sequence warmed, then blocks of back-to-back calls between ONE event pair (the sequences
with a read-back: wall clock around the block), `--repeats` blocks each, the sequences taking turns; median, minimum and maximum per
call over the blocks.

  python tools/amu_bench.py --out profiles/amu.json
  python tools/amu_bench.py --case opf_10000          (one case, JSON on stdout)
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


def one(case, block, repeats):
    import numpy as np
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib, transcribe, workloads
    from infiniteexamodels.jl_amd.barrier import AdaptiveBarrierParameter, BarrierLayer, BarrierParameter
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
    sol = T(1e-3 * rng.standard_normal(n + m))
    dirs = (T(1e-3 * rng.standard_normal(m)), T(1e-3 * rng.standard_normal(n)), T(1e-3 * rng.standard_normal(n)), T(1e-3 * rng.standard_normal(m)),
            T(1e-3 * rng.standard_normal(m)))
    alpha = T([0.75, 0.5])
    nz = info["nz"]
    # algorithmic bytes: flags, then what each kernel reads per entry and per present bound (8-byte words)
    with_x, with_s = int((hasL | hasU).sum()), int((gL | gU).sum())
    bytes_error = (n + m) + 8 * (2 * n + 2 * m + info["n_ineq"] + info["n_eq"] + 2 * nz)
    bytes_probe = (n + m) + 8 * (2 * with_x + 2 * with_s + 3 * nz)
    res = {"case": case, "model": MODELS[case], "device": torch.cuda.get_device_name(0), "repeats": repeats, "calls_per_block": block, **info,
           "bytes": {"mu_error": bytes_error, "amu_probe": bytes_probe, "probe_over_error": bytes_probe / bytes_error}}

    with BarrierLayer(gm, relax=RELAX) as bar, BarrierParameter(bar, mu_init=MU) as par, AdaptiveBarrierParameter(par) as amu:
        w12, q4 = gm._new(12), gm._new(4)
        par.error(state, rd, cd, out=w12)
        amu.probe(state, sol, dirs, alpha, out=q4)
        zero = tuple(torch.zeros_like(d) for d in dirs)
        q0 = amu.probe(state, torch.zeros_like(sol), zero, T([1.0, 1.0]))
        torch.cuda.synchronize()
        assert torch.equal(q0[:1].view(torch.int64), w12[9:10].view(torch.int64)), "the probe at zero directions is not word 9 of iem_mu_error"
        bd = {k: T(np.where(np.isfinite(parts[k]), parts[k], 0.0)) for k in ("xl", "xu", "rl", "ru")}
        on = {k: torch.tensor(v, device="cuda") for k, v in (("xL", hasL), ("xU", hasU), ("sL", gL), ("sU", gU))}
        zero_n, zero_m = torch.zeros(n, dtype=torch.float64, device="cuda"), torch.zeros(m, dtype=torch.float64, device="cuda")

        def rule():
            amu.probe(state, sol, dirs, alpha, out=q4)
            amu.update(w12, q4)
            return amu.state()

        def by_torch():
            xs, ss, _, zL, zU, vL, vU = state
            ds, dzL, dzU, dvL, dvU = dirs
            ap, ad = alpha[0], alpha[1]
            tx, ts = ap * sol[:n], ap * ds
            p = torch.cat([torch.where(on["xL"], ((xs - bd["xl"]) + tx) * (zL + ad * dzL), zero_n), torch.where(on["xU"], ((bd["xu"] - xs) - tx) * (zU + ad * dzU), zero_n),
                           torch.where(on["sL"], ((ss - bd["rl"]) + ts) * (vL + ad * dvL), zero_m), torch.where(on["sU"], ((bd["ru"] - ss) - ts) * (vU + ad * dvU), zero_m)])
            total, bad, w9 = torch.stack([p.sum(), torch.isnan(p).sum().to(torch.float64), w12[9]]).tolist()      # THE read-back
            if nz == 0:
                return 1e-11, bad
            avg = w9 / nz
            q = (total / nz) / avg
            return min(max(min(q * q * q, 100.0) * avg, 1e-11), 1e3 * avg), bad
        st = rule()
        mu_t, bad_t = by_torch()
        assert st["status_name"] == "iterating" and bad_t == 0.0 and abs(st["mu"] - mu_t) <= 1e-9 * abs(mu_t), (st, mu_t)
        calls = {"mu_error": lambda: par.error(state, rd, cd, out=w12), "amu_probe": lambda: amu.probe(state, sol, dirs, alpha, out=q4),
                 "amu_update": lambda: amu.update(w12, q4), "rule": rule, "torch": by_torch}

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
        res["us_per_call"] = timed(["mu_error", "amu_probe", "amu_update"], block, wall=False)
        res["amu_probe_over_mu_error"] = res["us_per_call"]["amu_probe"]["us_median"] / res["us_per_call"]["mu_error"]["us_median"]
        res["us_per_iteration_wall_clock"] = timed(["rule", "torch"], max(2, block // 2), wall=True)
        w = res["us_per_iteration_wall_clock"]
        res["torch_over_rule"] = w["torch"]["us_median"] / w["rule"]["us_median"]
    gm.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=CASES)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--block", type=int, default=100, help="calls between one event pair (half of it for the sequences with a read-back)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per case (child process)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "amu.json"))
    a = ap.parse_args()
    if a.case:
        print(json.dumps(one(a.case, a.block, a.repeats)))
        return 0
    doc = {"what": "tools/amu_bench.py: µs per call of iem_mu_error, iem_amu_probe (six direction vectors more, no logarithm, two reduced values) and iem_amu_update — "
                   "device events around blocks of back-to-back calls — with the algorithmic bytes of both grid kernels, and µs per 'probe + rule + read-back' — wall clock "
                   "around blocks: iem_amu_probe + iem_amu_update + iem_amu_state against the probe's sum and NaN count by torch expressions, one read-back, the rule on "
                   "the host; warm, the sequences taking turns; median / min / max over the blocks",
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
