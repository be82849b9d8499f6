#!/usr/bin/env python3
"""Durations of the explicit θ blocks in COO (jacp_coord, hessp_coord) beside their algorithmic bytes, and beside the
matrix-free kinds they replace (jpprod, hpprod, hptprod) from the same run; at 1e5 quadrotor supports also
sensitivity.parameter_jacobian against parameter_steps with unit directions for K = 16 columns through a ChainKKT.

Per case one child process under its own `timeout` (the parent never opens the GPU and stops at the first child that
fails): every call is warmed, then timed in blocks of back-to-back launches between one event pair, alternating the calls,
`--repeats` blocks each; median, minimum and maximum per call.  The bytes are the generator's own account
(iem_kernel_info: alg_bytes_read / alg_bytes_written summed over the kernels of the call).

  python tools/param_coord_bench.py --out profiles/param_coord.json
  python tools/param_coord_bench.py --case quadrotor_100000          (one case, JSON on stdout)
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
CALLS = ("jacp_coord", "hessp_coord", "jpprod", "hpprod", "hptprod")
COPY_RATE = 6.3e12      # bytes / s: the copy rate the hardware guide gives for the MI355X


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
    nj, nx, npp = gm.param_coord_nnz()
    rng = np.random.default_rng(0)
    xd = torch.tensor(gm.meta.x0 + 0.1 * rng.standard_normal(n), device="cuda")
    yd, wd, ud = (torch.tensor(rng.standard_normal(k), device="cuda") for k in (mc, npar, n))
    new = lambda k: [torch.empty(max(k, 1), dtype=torch.float64, device="cuda") for _ in range(3)]
    bufs = {"jacp_coord": new(nj), "hessp_coord": new(nx), "hessp_pp": new(npp), "jpprod": new(mc), "hpprod": new(n), "hptprod": new(npar)}
    p = lambda a: C.c_void_p(a.data_ptr())
    L, h = gm._L, gm._h
    gm.param_prepare()
    gm.param_coord_prepare()
    gm._sync_stream()
    call = {"jacp_coord": lambda r: L.iem_jacp_coord(h, p(xd), p(bufs["jacp_coord"][r])),
            "hessp_coord": lambda r: L.iem_hessp_coord(h, p(xd), p(yd), 1.0, p(bufs["hessp_coord"][r]), p(bufs["hessp_pp"][r])),
            "jpprod": lambda r: L.iem_jpprod(h, p(xd), p(wd), p(bufs["jpprod"][r])),
            "hpprod": lambda r: L.iem_hpprod(h, p(xd), p(yd), 1.0, p(wd), p(bufs["hpprod"][r])),
            "hptprod": lambda r: L.iem_hptprod(h, p(xd), p(yd), 1.0, p(ud), p(bufs["hptprod"][r]))}
    for k in CALLS:
        for r in range(3):
            for _ in range(30):
                iemlib.check(call[k](r))
    torch.cuda.synchronize()
    us = {k: [] for k in CALLS}
    for rep in range(repeats):
        for k in CALLS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                call[k](rep % 3)
            e1.record(); torch.cuda.synchronize()
            us[k].append(e0.elapsed_time(e1) / launches * 1e3)
    kernels = gm.param_kernels() + gm.param_coord_kernels()
    prefix = {"jacp_coord": "iem_jacp", "hessp_coord": "iem_hessp", "jpprod": "iem_jpprod", "hpprod": "iem_hpprod", "hptprod": "iem_hptprod"}
    res = {"case": case, "nvar": n, "ncon": mc, "npar": npar, "nnz_jacp_hessxp_hesspp": [nj, nx, npp], "launches_per_block": launches, "repeats": repeats,
           "jit": bool(any(k["jit"] for k in gm.kernels() + kernels)), "device": torch.cuda.get_device_name(0), "calls": {}}
    for k in CALLS:
        mine = [q for q in kernels if q["name"].startswith(prefix[k])]
        rb, wb = sum(q["alg_bytes_read"] for q in mine), sum(q["alg_bytes_written"] for q in mine)
        med = float(np.median(us[k]))
        res["calls"][k] = {"us_median": round(med, 3), "us_min": round(min(us[k]), 3), "us_max": round(max(us[k]), 3),
                           "kernels": [q["name"] for q in mine], "workgroups": [int(np.prod(q["grid"])) for q in mine],
                           "alg_bytes_read": rb, "alg_bytes_written": wb, "alg_GBps_at_median": round((rb + wb) / med * 1e-3, 1) if med > 0 else None,
                           "us_of_the_bytes_at_copy_rate": round((rb + wb) / COPY_RATE * 1e6, 3),
                           "median_over_copy_rate_time": round(med / ((rb + wb) / COPY_RATE * 1e6), 2) if rb + wb else None}
    if case == "quadrotor_100000":      # the consumer: K = 16 columns of d(x, y)/dθ through a factorised chain KKT system
        from infiniteexamodels.jl_amd.kkt import KKTSystem
        from infiniteexamodels.jl_amd.kkt_chain import ChainKKT
        from infiniteexamodels.jl_amd.sensitivity import parameter_jacobian, parameter_steps
        kkt = KKTSystem(gm)
        ck = ChainKKT(kkt)
        kkt.assemble(gm.hess_coord(xd, yd, obj_weight=1.0), gm.jac_coord(xd), torch.tensor(0.5 + rng.random(n), device="cuda"), 1e-2, 1e-6)
        ck.load().factor()
        cols = [int(c) for c in np.linspace(0, npar - 1, 16).astype(np.int64)]
        D = torch.zeros(npar, 16, dtype=torch.float64, device="cuda")
        for j, c in enumerate(cols):
            D[c, j] = 1.0
        paths = {"parameter_jacobian": lambda: parameter_jacobian(gm, ck, xd, yd, cols), "parameter_steps": lambda: parameter_steps(gm, ck, xd, yd, D)}
        for f in paths.values():
            for _ in range(5):
                f()
        torch.cuda.synchronize()
        t = {k: [] for k in paths}
        for rep in range(repeats):
            for k, f in paths.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(10):
                    f()
                e1.record(); torch.cuda.synchronize()
                t[k].append(e0.elapsed_time(e1) / 10 * 1e3)
        a, b = paths["parameter_jacobian"](), paths["parameter_steps"]()
        diff = float(max((a[0] - b[0]).abs().max(), (a[1] - b[1]).abs().max()) / max(1.0, float(b[0].abs().max()), float(b[1].abs().max())))
        res["sensitivity_matrix_K16"] = {k: {"us_median": round(float(np.median(v)), 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1)} for k, v in t.items()}
        res["sensitivity_matrix_K16"]["max_relative_difference"] = diff
        res["sensitivity_matrix_K16"]["note"] = "whole calls on the host's clock of launches: right-hand side and one ChainKKT.solve with 16 columns, 10 calls per block"
        kkt.close()
    gm.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--timeout", type=int, default=400, help="seconds per case (child process)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "param_coord.json"))
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
        print(case, {k: v["us_median"] for k, v in results[-1]["calls"].items()}, "us", results[-1].get("sensitivity_matrix_K16", ""), flush=True)
    doc = {"what": "tools/param_coord_bench.py: per-call time of the explicit θ blocks in COO and of the matrix-free kinds beside them (device events "
                   "around blocks of back-to-back launches, warm; median / min / max over the blocks), the algorithmic bytes iem_kernel_info reports "
                   "for their kernels and the time those bytes take at 6.3 TB/s",
           "cases": results}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
