#!/usr/bin/env python3
"""What a product with the KKT matrix costs, and what refinement adds to a solve, in the same run on one handle.

  a  kktprod                                     iem_kktprod: W·u + Jᵀ·v and J·u from one launch
  b  hprod + jtprod + jprod + add                today's matrix-free product: three generated launches and a torch add
  c  ChainKKT._matvec                            today's refinement product: iem_csr_spmv on the CSR copy of K
  d  iem_kkt_solve                               one pass through the chain solver's factors
  e  iem_kkt_solve_refined(steps = 1)            solve, matrix-free residual, solve, add (no norms)

Per case one child process under its own `timeout` (the parent never opens the GPU and stops at the first child that fails): a, b
and c are checked against each other at the same (x, y, u, v) — the CSR matrix assembled without diagonal terms, so that all
three are the product with [W, Jᵀ; J, 0] — then every sequence is warmed and timed in blocks of back-to-back repetitions between
one event pair, the sequences taking turns, `--repeats` blocks each; median, minimum and maximum per repetition.  The bytes are
the generator's own account (iem_kernel_info: alg_bytes_read / alg_bytes_written of the kernels a sequence launches; the torch add
of b is in the time, not in the bytes; c moves 12 bytes per stored entry of K plus the vectors; d and e have no such account).

  python tools/kktprod_bench.py --out profiles/kktprod.json
  python tools/kktprod_bench.py --case quadrotor_100000          (one case, JSON on stdout)
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"quadrotor_100000": 100_000, "quadrotor_1000000": 1_000_000}
SEQS = ("a kktprod", "b hprod+jtprod+jprod+add", "c ChainKKT._matvec (CSR)", "d iem_kkt_solve", "e iem_kkt_solve_refined(steps=1)")
TOL = 1e-10


def one(case, launches, solve_launches, repeats):
    import numpy as np
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib, transcribe, workloads
    from infiniteexamodels.jl_amd.kkt import KKTSystem
    from infiniteexamodels.jl_amd.kkt_chain import ChainKKT
    from infiniteexamodels.jl_amd.model import ExaModel
    gm = ExaModel(transcribe.exa_core(workloads.quadrotor(CASES[case])), device=0)
    n, mc = gm.meta.nvar, gm.meta.ncon
    rng = np.random.default_rng(0)
    dev = lambda a: torch.tensor(a, device="cuda")
    xd, yd = dev(gm.meta.x0 + 0.1 * rng.standard_normal(n)), dev(rng.standard_normal(mc))
    z = dev(rng.standard_normal(n + mc))
    ud, vd = z[:n], z[n:]
    new = lambda k: torch.empty(max(k, 1), dtype=torch.float64, device="cuda")
    ka, hu, jtv = new(n + mc), new(n), new(n)
    kb = new(n + mc)
    p = lambda a: C.c_void_p(a.data_ptr())
    L, h = gm._L, gm._h
    gm.kkt_prepare()
    # c: the CSR copy of K0 = [W, J'; J, 0] (no diagonal terms: the three products are comparable)
    hv, jv = gm.hess_coord(xd, yd, obj_weight=1.0), gm.jac_coord(xd)
    kk = KKTSystem(gm)
    kk.assemble(hv, jv, None, 0.0, 0.0)
    csr = types.SimpleNamespace(kkt=kk, model=gm, _torch=torch, _long_rows=None)
    out = {}
    # d, e: the solver object, regularised like an interior-point iterate
    sd = dev(0.5 + rng.random(n))
    dw, dc = 1e-2, 1e-6
    k = C.c_void_p()
    iemlib.check(L.iem_kkt_create(h, 0, C.byref(k)))
    gm._sync_stream()
    iemlib.check(L.iem_kkt_assemble(k, p(hv), p(jv), p(sd), dw, dc))
    inertia = (C.c_int64 * 3)()
    iemlib.check(L.iem_kkt_factor(k, inertia))
    rhs, sol_d, sol_e, norms = dev(rng.standard_normal(n + mc)), new(n + mc), new(n + mc), new(2)

    def seq_a():
        iemlib.check(L.iem_kktprod(h, p(xd), p(yd), 1.0, p(ud), p(vd), p(ka), C.c_void_p(ka.data_ptr() + 8 * n)))

    def seq_b():
        iemlib.check(L.iem_hprod(h, p(xd), p(yd), p(ud), 1.0, p(hu)))
        iemlib.check(L.iem_jtprod(h, p(xd), p(vd), p(jtv)))
        iemlib.check(L.iem_jprod(h, p(xd), p(ud), C.c_void_p(kb.data_ptr() + 8 * n)))
        torch.add(hu, jtv, out=kb[:n])

    def seq_c():
        out["c"] = ChainKKT._matvec(csr, z)

    def seq_d():
        iemlib.check(L.iem_kkt_solve(k, p(rhs), p(sol_d)))

    def seq_e():
        iemlib.check(L.iem_kkt_solve_refined(k, p(xd), p(yd), 1.0, p(sd), dw, dc, p(rhs), p(sol_e), 1, None))

    seqs = dict(zip(SEQS, (seq_a, seq_b, seq_c, seq_d, seq_e)))
    # the three products agree before anything is timed; the refined solve leaves the smaller residual
    seq_a(); seq_b(); seq_c(); torch.cuda.synchronize()
    scale = max(1.0, float(kb.abs().max().item()))
    agree = {"a vs b": float((ka - kb).abs().max().item()) / scale, "c vs b": float((out["c"] - kb).abs().max().item()) / scale}
    assert max(agree.values()) <= TOL, f"the three products disagree: {agree}"
    assert torch.equal(ka[n:].view(torch.int64), kb[n:].view(torch.int64)), "kktprod's rows are not iem_jprod's to the bit"
    seq_d(); seq_e()
    iemlib.check(L.iem_kkt_residual(k, p(xd), p(yd), 1.0, p(sd), dw, dc, p(rhs), p(sol_d), p(new(n + mc)), p(norms[:1])))
    iemlib.check(L.iem_kkt_residual(k, p(xd), p(yd), 1.0, p(sd), dw, dc, p(rhs), p(sol_e), p(new(n + mc)), p(norms[1:])))
    torch.cuda.synchronize()
    res_norms = [float(v) for v in norms.tolist()]
    per_block = {s: (solve_launches if s[0] in "de" else launches) for s in SEQS}
    for s in SEQS:
        for _ in range(20 if s[0] in "abc" else 3):
            seqs[s]()
    torch.cuda.synchronize()
    us = {s: [] for s in SEQS}
    for _ in range(repeats):
        for s in SEQS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(per_block[s]):
                seqs[s]()
            e1.record(); torch.cuda.synchronize()
            us[s].append(e0.elapsed_time(e1) / per_block[s] * 1e3)
    own, mine = gm.kernels(), gm.kkt_kernels()
    kind = lambda ks, kd: [q for q in ks if q["kind"] == kd]
    launched = dict(zip(SEQS, (kind(mine, "trial") or kind(mine, "jprod") + kind(mine, "hprod"), kind(own, "hprod") + kind(own, "jtprod") + kind(own, "jprod"), [], [], [])))
    res = {"case": case, "nvar": n, "ncon": mc, "nnz_csr": int(kk.nnz), "launches_per_block": per_block, "repeats": repeats,
           "jit": bool(any(q["jit"] for q in own + mine)), "device": torch.cuda.get_device_name(0), "products_agree_rel": agree,
           "inertia": list(inertia), "residual_max_unrefined": res_norms[0], "residual_max_refined_1": res_norms[1], "sequences": {}}
    for s in SEQS:
        ks = launched[s]
        med = float(np.median(us[s]))
        res["sequences"][s] = {"us_median": round(med, 3), "us_min": round(min(us[s]), 3), "us_max": round(max(us[s]), 3),
                               "kernels": [q["name"] for q in ks], "workgroups": [int(np.prod(q["grid"])) for q in ks],
                               "alg_bytes_read": sum(q["alg_bytes_read"] for q in ks), "alg_bytes_written": sum(q["alg_bytes_written"] for q in ks)}
    # c by its own count: value + 32-bit column per stored entry, a row pointer per row, z read and the result written
    res["sequences"][SEQS[2]]["alg_bytes_read"] = 12 * int(kk.nnz) + 4 * (n + mc + 1) + 8 * (n + mc)
    res["sequences"][SEQS[2]]["alg_bytes_written"] = 8 * (n + mc)
    m = {s[0]: res["sequences"][s]["us_median"] for s in SEQS}
    res["order"] = {"a < b": m["a"] < m["b"], "a < c": m["a"] < m["c"]}
    iemlib.check(L.iem_kkt_destroy(k))
    kk.close()
    gm.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--launches", type=int, default=50, help="repetitions per block of the products a, b, c")
    ap.add_argument("--solve-launches", type=int, default=5, help="repetitions per block of the solves d, e")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=420, help="seconds per case (child process)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kktprod.json"))
    a = ap.parse_args()
    if a.case:
        print(json.dumps(one(a.case, a.launches, a.solve_launches, a.repeats)))
        return 0
    doc = {"what": "tools/kktprod_bench.py: per-repetition time of the product with the KKT matrix from iem_kktprod, from today's three "
                   "generated products plus a torch add and from the CSR copy of K, and of a solve with and without one matrix-free "
                   "refinement step; device events around blocks of back-to-back repetitions, warm; median / min / max over the "
                   "blocks, beside the algorithmic bytes iem_kernel_info reports for the generated kernels each sequence launches",
           "cases": []}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for case in a.cases.split(","):
        r = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--case", case,
                            "--launches", str(a.launches), "--solve-launches", str(a.solve_launches), "--repeats", str(a.repeats)],
                           stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            print(f"{case}: FAILED with exit status {r.returncode}; nothing more is started", file=sys.stderr)
            return 1
        doc["cases"].append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(case, {k: v["us_median"] for k, v in doc["cases"][-1]["sequences"].items()}, "us", doc["cases"][-1]["order"], flush=True)
        with open(a.out, "w") as f:      # after every case: what was measured stays if a later case fails
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
