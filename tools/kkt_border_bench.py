#!/usr/bin/env python3
"""The dense border on the host (mode 0) against the device (mode 1, iem_kkt_set_border), through the C-ABI object, on one MI355X.

Per model (pandemic 110 x 128: ne = 112; stochastic OPF, 1e4 scenarios; farmer, 1e5 scenarios) and call (iem_kkt_assemble + iem_kkt_factor,
iem_kkt_solve, iem_kkt_solve_many(16), iem_kkt_solve_refined(1)): the time per call in both modes IN ONE PROCESS, the modes
alternating repeat by repeat.  A repeat is a block of calls between a device synchronise and the next, on the host clock (mode 0
works on the host inside the call: device events alone would not see where that time goes); the median and the spread (min ..
max) of the repeats are reported.  Beside them the two border launches on their own at the model's border size — the low-level
iem_kkt_border_factor / iem_kkt_border_solve with S = 1 (two one-block column-sum launches in front of the kernel), between device
events.

    python tools/kkt_border_bench.py [--models pandemic,opf,farmer] [--out profiles/kkt_border.json]"""
import argparse, ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from infiniteexamodels.jl_amd import lib as iemlib, transcribe, workloads
from infiniteexamodels.jl_amd.model import ExaModel

ap = argparse.ArgumentParser()
ap.add_argument("--models", default="pandemic,opf,farmer")
ap.add_argument("--block", type=int, default=5, help="calls per repeat")
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--opf", type=int, default=10_000)
ap.add_argument("--farmer", type=int, default=100_000)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kkt_border.json"))
args = ap.parse_args()
MODELS = {"pandemic": lambda: workloads.pandemic(100, 128), "opf": lambda: workloads.opf(args.opf), "farmer": lambda: workloads.farmer(args.farmer)}
p = lambda t: C.c_void_p(t.data_ptr())
DW, DC = 1e-2, 1e-6


def block_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.block):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / args.block


def event_ms(fn):
    fn(); fn(); torch.cuda.synchronize()
    out = []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.block):
            fn()
        e1.record(); torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / args.block)
    return summary(out)


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


results = {"tool": "tools/kkt_border_bench.py (ms per call; %d calls per repeat between two synchronisations on the host clock, %d repeats, the modes alternating: median, min, max)"
                   % (args.block, args.repeats), "device": torch.cuda.get_device_name(0), "models": {}}
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
    S, nb, ne, nc, n_border = int(info.S), int(info.nb), int(info.ne), int(info.nc), int(info.n_border)
    assert ne > 0 and not info.hubs, "a model with a dense border is wanted here"
    gm._sync_stream()
    inertia = (C.c_int64 * 3)()
    rhs = torch.tensor(rng.standard_normal((16, n)), device="cuda")
    sol = torch.empty_like(rhs)
    norms = torch.empty(2, dtype=torch.float64, device="cuda")

    def factor():      # (with its assemble: the factorisation works in place)
        iemlib.check(L_.iem_kkt_assemble(k, p(hv), p(jv), p(sigma), DW, DC))
        iemlib.check(L_.iem_kkt_factor(k, inertia))

    calls = {"assemble_factor": factor,
             "solve": lambda: iemlib.check(L_.iem_kkt_solve(k, p(rhs[0]), p(sol[0]))),
             "solve_many_16": lambda: iemlib.check(L_.iem_kkt_solve_many(k, 16, p(rhs), n, p(sol), n)),
             "solve_refined_1": lambda: iemlib.check(L_.iem_kkt_solve_refined(k, p(x), p(y), 1.0, p(sigma), DW, DC, p(rhs[1]), p(sol[1]), 1, p(norms)))}
    times = {c: {0: [], 1: []} for c in calls}
    inert, first = {}, {}
    for rep in range(args.repeats + 1):      # (repeat 0 is the warm-up of both modes: code objects, workspaces)
        for mode in (0, 1):
            iemlib.check(L_.iem_kkt_set_border(k, mode))
            factor()
            inert[mode] = [int(v) for v in inertia]
            for c, fn in calls.items():
                fn()
                t = block_ms(fn)
                if rep:
                    times[c][mode].append(t)
            first[mode] = sol[0].clone()
    # the two border launches on their own, at this border size
    G = torch.eye(ne, dtype=torch.float64, device="cuda") * 4.0 + torch.tensor(rng.standard_normal((ne, ne)), device="cuda")
    G = G + G.t()
    Gp = torch.zeros(1, ne, ne, dtype=torch.float64, device="cuda")
    F, piv = torch.empty(ne, ne, dtype=torch.float64, device="cuda"), torch.empty(ne, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(3, dtype=torch.int64, device="cuda")
    rBp, rB, xB = (torch.tensor(rng.standard_normal((4, ne)), device="cuda") for _ in range(3))
    ldl = event_ms(lambda: iemlib.check(L_.iem_kkt_border_factor(gm._h, 1, ne, n_border, p(G), p(Gp), p(F), p(piv), p(cnt), 1e-14)))
    sub1 = event_ms(lambda: iemlib.check(L_.iem_kkt_border_solve(gm._h, 1, ne, n_border, 1, p(F), p(piv), p(rBp), p(rB), p(xB))))
    sub4 = event_ms(lambda: iemlib.check(L_.iem_kkt_border_solve(gm._h, 1, ne, n_border, 4, p(F), p(piv), p(rBp), p(rB), p(xB))))
    rows = {}
    for c in calls:
        m0, m1 = summary(times[c][0]), summary(times[c][1])
        rows[c] = {"mode0_ms": m0, "mode1_ms": m1, "mode0_over_mode1": m0["median"] / m1["median"]}
        print(name, c, "mode 0 %.3f [%.3f .. %.3f]" % (m0["median"], m0["min"], m0["max"]), "mode 1 %.3f [%.3f .. %.3f] ms" % (m1["median"], m1["min"], m1["max"]), flush=True)
    diff = float((first[0] - first[1]).abs().max().item() / max(1.0, first[0].abs().max().item()))
    results["models"][name] = {"n": n, "S": S, "nb": nb, "ne": ne, "nc": nc, "n_border": n_border, "inertia_mode0": inert[0], "inertia_mode1": inert[1],
                               "solution_mode1_against_mode0_relative": diff, "calls": rows,
                               "border_launches_alone_ms": {"factor_S1": ldl, "solve_S1_nrhs1": sub1, "solve_S1_nrhs4": sub4}}
    print(name, "border launches alone: ldl %.4f, solve %.4f, solve x 4 %.4f ms" % (ldl["median"], sub1["median"], sub4["median"]), flush=True)
    iemlib.check(L_.iem_kkt_destroy(k))
    gm.close()
    del gm, hv, jv, rhs, sol
    torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:      # (after every model: a later one failing keeps the earlier rows)
        json.dump(results, f, indent=1)
print(json.dumps(results))
