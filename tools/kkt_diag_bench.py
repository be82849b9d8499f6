#!/usr/bin/env python3
"""What the per-row diagonal costs at assembly, and what the multi-column refined solve costs per column, on one KKT object.

  a0  iem_kkt_assemble                                      scalar delta_c (kkt_gather_d without dcon)
  a1  iem_kkt_assemble_diag with a vector dcon              the same kernel: 8·ncon bytes more to read
  b0  16 x iem_kkt_solve_refined(steps = 1)                 per column: solve, operator, finishing kernel, solve, add
  b1  iem_kkt_solve_refined_diag(nrhs = 16, steps = 1)      iem_kkt_solve_many for the solves, the same operator launches, one
                                                            finishing launch and one add per slab of 8 columns

Both b sequences run on the scalar-delta_c matrix (d_dcon = NULL), without norms.  Per model one child process under its own
`timeout` (the parent never opens the GPU and stops at the first child that fails).  The method is that of tools/kktprod_bench.py:
every sequence warmed, then blocks of back-to-back calls between one event pair, `--repeats` blocks each, the two sequences of a
pair taking turns on ONE object; median, minimum and maximum per call.  Assembling invalidates the factors, so the a pair is timed
first, then the object is factorised once for the b pair.  Bordered models run in border mode 1 (no host step inside a solve).

  python tools/kkt_diag_bench.py --out profiles/kkt_diag.json
  python tools/kkt_diag_bench.py --case opf_10000          (one case, JSON on stdout)
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ("quadrotor_100000", "opf_10000", "pandemic_110x128")
NRHS = 16
DW, DC = 1e-2, 1e-6


def one(case, asm_block, solve_block, repeats):
    import numpy as np
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib, transcribe, workloads
    from infiniteexamodels.jl_amd.model import ExaModel
    make = {"quadrotor_100000": lambda: workloads.quadrotor(100_000), "opf_10000": lambda: workloads.opf(10_000), "pandemic_110x128": lambda: workloads.pandemic(100, 128)}[case]
    gm = ExaModel(transcribe.exa_core(make()), device=0)
    L, nvar, ncon = gm._L, gm.meta.nvar, gm.meta.ncon
    n = nvar + ncon
    rng = np.random.default_rng(0)
    dev = lambda a: torch.tensor(a, device="cuda")
    p = lambda a: C.c_void_p(a.data_ptr()) if a is not None else None
    x0 = gm.meta.x0 + 0.1 * rng.standard_normal(nvar)
    xd = dev(np.abs(x0) + 0.05 if case.startswith("pandemic") else x0)
    yd = dev(0.1 * np.random.default_rng(1).standard_normal(ncon))
    sd = dev(0.5 + rng.random(nvar))
    dcon = dev(np.where(rng.random(ncon) < 0.5, 10.0 ** rng.uniform(-8.0, 8.0, ncon), 0.0))
    hv, jv = gm.hess_coord(xd, yd), gm.jac_coord(xd)
    gm.kkt_prepare()
    k = C.c_void_p()
    iemlib.check(L.iem_kkt_create(gm._h, 0, C.byref(k)))
    info = iemlib.KktInfo()
    iemlib.check(L.iem_kkt_info(k, C.byref(info)))
    gm._sync_stream()
    iemlib.check(L.iem_kkt_set_border(k, 1))
    rhs = dev(rng.standard_normal((NRHS, n)))
    sol0, sol1 = torch.empty_like(rhs), torch.empty_like(rhs)
    inertia = (C.c_int64 * 3)()

    def a0():
        iemlib.check(L.iem_kkt_assemble(k, p(hv), p(jv), p(sd), DW, DC))

    def a1():
        iemlib.check(L.iem_kkt_assemble_diag(k, p(hv), p(jv), p(sd), p(dcon), DW, DC))

    def b0():
        for u in range(NRHS):
            iemlib.check(L.iem_kkt_solve_refined(k, p(xd), p(yd), 1.0, p(sd), DW, DC, p(rhs[u]), p(sol0[u]), 1, None))

    def b1():
        iemlib.check(L.iem_kkt_solve_refined_diag(k, p(xd), p(yd), 1.0, p(sd), None, DW, DC, NRHS, p(rhs), n, p(sol1), n, 1, None))

    def pair(f, g, block, warm):
        for fn in (f, g):
            for _ in range(warm):
                fn()
        torch.cuda.synchronize()
        ms = ([], [])
        for _ in range(repeats):
            for which, fn in enumerate((f, g)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(block):
                    fn()
                e1.record(); torch.cuda.synchronize()
                ms[which].append(e0.elapsed_time(e1) / block)
        return [{"ms_median": float(np.median(v)), "ms_min": min(v), "ms_max": max(v)} for v in ms]

    # the vector's matrix factorises with the inertia of a regularised system before anything is timed
    a1()
    iemlib.check(L.iem_kkt_factor(k, inertia))
    inertia_diag = [int(v) for v in inertia]
    ta0, ta1 = pair(a0, a1, asm_block, 5)
    a0()
    iemlib.check(L.iem_kkt_factor(k, inertia))
    b0(); b1(); torch.cuda.synchronize()
    assert torch.equal(sol0.view(torch.int64), sol1.view(torch.int64)), "a column of the multi-column refined solve is not the single refined solve to the bit"
    tb0, tb1 = pair(b0, b1, solve_block, 2)
    res = {"case": case, "nvar": nvar, "ncon": ncon, "S": int(info.S), "nb": int(info.nb), "ne": int(info.ne), "nc": int(info.nc), "hubs": int(info.hubs),
           "block_doubles": int(info.block_doubles), "device": torch.cuda.get_device_name(0), "repeats": repeats,
           "calls_per_block": {"assemble": asm_block, "solve": solve_block}, "inertia_scalar": [int(v) for v in inertia], "inertia_diag": inertia_diag,
           "a0 iem_kkt_assemble": ta0, "a1 iem_kkt_assemble_diag(vector)": ta1,
           "b0 16 x iem_kkt_solve_refined(steps=1), per column": {q: v / NRHS for q, v in tb0.items()},
           "b1 iem_kkt_solve_refined_diag(nrhs=16, steps=1), per column": {q: v / NRHS for q, v in tb1.items()}}
    spread = max(ta0["ms_max"] - ta0["ms_min"], ta1["ms_max"] - ta1["ms_min"])
    res["demands"] = {"a: |a1 - a0| within the spread of the blocks": abs(ta1["ms_median"] - ta0["ms_median"]) <= spread,
                      "b: per column below the single refined solve": tb1["ms_median"] < tb0["ms_median"]}
    iemlib.check(L.iem_kkt_destroy(k))
    gm.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=CASES)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--assemble-block", type=int, default=20)
    ap.add_argument("--solve-block", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=420, help="seconds per case (child process)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kkt_diag.json"))
    a = ap.parse_args()
    if a.case:
        print(json.dumps(one(a.case, a.assemble_block, a.solve_block, a.repeats)))
        return 0
    doc = {"what": "tools/kkt_diag_bench.py: ms per call of iem_kkt_assemble against iem_kkt_assemble_diag with a vector, and ms per column of "
                   "iem_kkt_solve_refined_diag(nrhs = 16, steps = 1) against 16 calls of iem_kkt_solve_refined(steps = 1), on one object per model; "
                   "device events around blocks of back-to-back calls, warm, the two sequences of a pair taking turns; median / min / max over the blocks",
           "cases": []}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for case in a.cases.split(","):
        r = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--case", case, "--assemble-block", str(a.assemble_block),
                            "--solve-block", str(a.solve_block), "--repeats", str(a.repeats)], stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            print(f"{case}: FAILED with exit status {r.returncode}; nothing more is started", file=sys.stderr)
            return 1
        doc["cases"].append(json.loads(r.stdout.strip().splitlines()[-1]))
        c = doc["cases"][-1]
        print(case, {q: round(v["ms_median"], 4) for q, v in c.items() if isinstance(v, dict) and "ms_median" in v}, "ms", c["demands"], flush=True)
        with open(a.out, "w") as f:      # after every case: what was measured stays if a later case fails
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
