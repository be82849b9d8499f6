#!/usr/bin/env python3
"""Durations of the five parameter kinds (jpprod, jptprod, hpprod, hptprod, hppprod) beside their algorithmic bytes.

Per case one child process under its own `timeout` (the parent never opens the GPU and stops at the first child that
fails): every kind is warmed, then timed in blocks of back-to-back launches between one event pair, alternating the kinds,
`--repeats` blocks each; median, minimum and maximum per call.  The bytes are the generator's own account
(iem_kernel_info: alg_bytes_read / alg_bytes_written summed over the kernels of the kind; follow-up launches — memsets,
axis sums, the plan-driven gather — are not in them but are in the time).

  python tools/param_kinds_bench.py --out profiles/hppprod.json          (profiles/param_kinds.json: the run before hppprod existed)
  python tools/param_kinds_bench.py --case quadrotor_100000          (one case, JSON on stdout)
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"quadrotor_100000": ("quadrotor", 100_000), "quadrotor_1000000": ("quadrotor", 1_000_000), "heat_400x401": ("heat", (400, 401))}
KINDS = ("jpprod", "jptprod", "hpprod", "hptprod", "hppprod")


def one(case, launches, repeats):
    import numpy as np
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib, transcribe, workloads
    from infiniteexamodels.jl_amd.model import ExaModel
    wl, size = CASES[case]
    im = workloads.quadrotor(size) if wl == "quadrotor" else workloads.heat(size[0], size[1], "central")
    core = transcribe.exa_core(im)
    gm = ExaModel(core, device=0)
    n, mc, npar = gm.meta.nvar, gm.meta.ncon, gm.meta.npar
    rng = np.random.default_rng(0)
    xd = torch.tensor(gm.meta.x0 + 0.1 * rng.standard_normal(n), device="cuda")
    yd, wd, ud = (torch.tensor(rng.standard_normal(k), device="cuda") for k in (mc, npar, n))
    outs = {"jpprod": mc, "jptprod": npar, "hpprod": n, "hptprod": npar, "hppprod": npar}
    bufs = {k: [torch.empty(max(v, 1), dtype=torch.float64, device="cuda") for _ in range(3)] for k, v in outs.items()}
    p = lambda a: C.c_void_p(a.data_ptr())
    L, h = gm._L, gm._h
    gm.param_prepare()
    gm.hppprod_prepare()
    gm._sync_stream()
    call = {"jpprod": lambda o: L.iem_jpprod(h, p(xd), p(wd), p(o)), "jptprod": lambda o: L.iem_jptprod(h, p(xd), p(yd), 1.0, p(o)),
            "hpprod": lambda o: L.iem_hpprod(h, p(xd), p(yd), 1.0, p(wd), p(o)), "hptprod": lambda o: L.iem_hptprod(h, p(xd), p(yd), 1.0, p(ud), p(o)),
            "hppprod": lambda o: L.iem_hppprod(h, p(xd), p(yd), 1.0, p(wd), p(o))}
    for k in KINDS:
        for o in bufs[k]:
            for _ in range(30):
                iemlib.check(call[k](o))
    torch.cuda.synchronize()
    us = {k: [] for k in KINDS}
    for r in range(repeats):
        for k in KINDS:
            o = bufs[k][r % 3]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                call[k](o)
            e1.record(); torch.cuda.synchronize()
            us[k].append(e0.elapsed_time(e1) / launches * 1e3)
    kernels = gm.param_kernels() + gm.hppprod_kernels()
    res = {"case": case, "nvar": n, "ncon": mc, "npar": npar, "launches_per_block": launches, "repeats": repeats,
           "jit": bool(any(k["jit"] for k in gm.kernels())), "device": torch.cuda.get_device_name(0), "kinds": {}}
    for k in KINDS:
        mine = [q for q in kernels if q["name"].startswith("iem_" + k)]
        rb, wb = sum(q["alg_bytes_read"] for q in mine), sum(q["alg_bytes_written"] for q in mine)
        med = float(np.median(us[k]))
        res["kinds"][k] = {"us_median": round(med, 3), "us_min": round(min(us[k]), 3), "us_max": round(max(us[k]), 3),
                           "kernels": [q["name"] for q in mine], "workgroups": [int(np.prod(q["grid"])) for q in mine],
                           "alg_bytes_read": rb, "alg_bytes_written": wb, "alg_GBps_at_median": round((rb + wb) / med * 1e-3, 1) if med > 0 else None,
                           "output_bytes": 8 * outs[k]}
    gm.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--timeout", type=int, default=400, help="seconds per case (child process)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hppprod.json"))
    a = ap.parse_args()
    if a.case:
        print(json.dumps(one(a.case, a.launches, a.repeats)))
        return 0
    results = []
    for case in a.cases.split(","):
        r = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--case", case,
                            "--launches", str(a.launches), "--repeats", str(a.repeats)], stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            print(f"{case}: FAILED with exit status {r.returncode}; nothing more is started", file=sys.stderr)
            return 1
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(case, {k: v["us_median"] for k, v in results[-1]["kinds"].items()}, "us", flush=True)
    doc = {"what": "tools/param_kinds_bench.py: per-call time of the parameter kinds (device events around blocks of back-to-back launches, warm; "
                   "median / min / max over the blocks) beside the algorithmic bytes iem_kernel_info reports for their kernels",
           "cases": results}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
