#!/usr/bin/env python3
"""iem_kkt_solve_many against back-to-back iem_kkt_solve calls, through the C-ABI object, on one MI355X.

Per model (quadrotor 1e5 supports, hovercraft 1e5, pandemic 110 x 128) and nrhs in {1, 2, 4, 8, 16}: the time of ONE
iem_kkt_solve_many(nrhs) and of nrhs iem_kkt_solve calls in the same process, each measured warm as a block of calls between
one pair of events, repeated; the median and the spread (min .. max) of the repeats are reported, per call and per column,
next to the byte model  (factor_bytes / R + vector_bytes) / 6.3 TB/s  per column (R = the shape's chunk width; factor_bytes =
D^-1 + Bt + BR + Z, vector_bytes = r + z).

    python tools/kkt_solve_many_bench.py [--models quadrotor,hovercraft,pandemic] [--out profiles/kkt_solve_many.json]"""
import argparse, ctypes as C, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from infiniteexamodels.jl_amd import lib as iemlib, transcribe, workloads
from infiniteexamodels.jl_amd.model import ExaModel

ap = argparse.ArgumentParser()
ap.add_argument("--models", default="quadrotor,hovercraft,pandemic")
ap.add_argument("--supports", type=int, default=100_000)
ap.add_argument("--block", type=int, default=5, help="calls between one pair of events")
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kkt_solve_many.json"))
args = ap.parse_args()
COPY_RATE = 6.3e12      # achieved device-to-device copy rate
NRHS = (1, 2, 4, 8, 16)
MODELS = {"quadrotor": lambda: workloads.quadrotor(args.supports), "hovercraft": lambda: workloads.hovercraft(args.supports),
          "pandemic": lambda: workloads.pandemic(100, 128)}      # 100 + 10 time supports x 128 scenarios: lanes, u(t) in the border
p = lambda t: C.c_void_p(t.data_ptr())


def timed(fn):
    """ms per call: warm, then `repeats` blocks of `block` calls, each between one pair of events."""
    fn(); fn(); torch.cuda.synchronize()
    out = []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.block):
            fn()
        e1.record(); torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / args.block)
    return {"median": statistics.median(out), "min": min(out), "max": max(out)}


results = {"tool": "tools/kkt_solve_many_bench.py (ms per call; blocks of %d calls between one event pair, %d repeats: median, min, max)" % (args.block, args.repeats),
           "device": torch.cuda.get_device_name(0), "copy_rate_bytes_per_s": COPY_RATE, "models": {}}
for name in args.models.split(","):
    core = transcribe.exa_core(MODELS[name]())
    gm = ExaModel(core, device=0)
    L_ = gm._L
    nvar, ncon = gm.meta.nvar, gm.meta.ncon
    n = nvar + ncon
    rng = np.random.default_rng(0)
    x0 = gm.meta.x0 + 0.1 * rng.standard_normal(nvar)
    x = torch.tensor(np.abs(x0) + 0.05 if name == "pandemic" else x0, device="cuda")
    y = torch.tensor(0.1 * np.random.default_rng(1).standard_normal(ncon), device="cuda")
    sigma = torch.tensor(0.5 + rng.random(nvar), device="cuda")
    hv, jv = gm.hess_coord(x, y), gm.jac_coord(x)
    k = C.c_void_p()
    iemlib.check(L_.iem_kkt_create(gm._h, 0, C.byref(k)))
    info = iemlib.KktInfo()
    iemlib.check(L_.iem_kkt_info(k, C.byref(info)))
    gm._sync_stream()
    iemlib.check(L_.iem_kkt_assemble(k, p(hv), p(jv), p(sigma), 1e-2, 1e-6))
    inertia = (C.c_int64 * 3)()
    iemlib.check(L_.iem_kkt_factor(k, inertia))
    S, nb, ne, nc = int(info.S), int(info.nb), int(info.ne), int(info.nc)
    R = iemlib.kkt_many_width(nb, ne, nc)
    factor_bytes = 8 * (S * nb * nb + 2 * S * nc * nc + S * nb * ne)
    vector_bytes = 8 * 2 * S * nb
    model_ms = (factor_bytes / R + vector_bytes) / COPY_RATE * 1e3
    rhs = torch.tensor(rng.standard_normal((max(NRHS), n)), device="cuda")
    sol = torch.empty_like(rhs)
    rows = {}
    for nk in NRHS:
        many = timed(lambda: iemlib.check(L_.iem_kkt_solve_many(k, nk, p(rhs), n, p(sol), n)))

        def singles():
            for u in range(nk):
                iemlib.check(L_.iem_kkt_solve(k, p(rhs[u]), p(sol[u])))
        one = timed(singles)
        rows[str(nk)] = {"solve_many_ms": many, "singles_ms": one,
                         "per_column_ms": {"solve_many": many["median"] / nk, "singles": one["median"] / nk},
                         "speedup": one["median"] / many["median"]}
        print(name, "nrhs", nk, "many %.3f [%.3f .. %.3f]" % (many["median"], many["min"], many["max"]),
              "singles %.3f [%.3f .. %.3f]" % (one["median"], one["min"], one["max"]), "ms;  per column %.3f against %.3f" % (many["median"] / nk, one["median"] / nk), flush=True)
    # the same bits either way (one column, checked here once more at scale)
    a = torch.empty(n, dtype=torch.float64, device="cuda")
    iemlib.check(L_.iem_kkt_solve(k, p(rhs[R + 1]), p(a)))
    iemlib.check(L_.iem_kkt_solve_many(k, max(NRHS), p(rhs), n, p(sol), n))
    torch.cuda.synchronize()
    at_R = rows[str(R)] if str(R) in rows else None
    results["models"][name] = {"n": n, "S": S, "nb": nb, "ne": ne, "nc": nc, "R": R, "inertia": [int(v) for v in inertia],
                               "factor_bytes": factor_bytes, "vector_bytes": vector_bytes, "byte_model_ms_per_column": model_ms,
                               "byte_model_over_measured_at_R": (model_ms / at_R["per_column_ms"]["solve_many"]) if at_R else None,
                               "column_equals_single_solve_bitwise": bool(torch.equal(a, sol[R + 1])), "nrhs": rows}
    iemlib.check(L_.iem_kkt_destroy(k))
    gm.close()
    del gm, hv, jv, rhs, sol
    torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:      # (after every model: a later one failing keeps the earlier rows)
        json.dump(results, f, indent=1)
print(json.dumps(results))
