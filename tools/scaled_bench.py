#!/usr/bin/env python3
"""What row scaling costs a solver, in the kernels and around them, in the same run on one handle.

  a  jac_coord                                   the unscaled call, for reference
  b  jac_coord + vals.mul_(s[rows])              today's scaled Jacobian (contrib/ipm.py: _Scaled.jac_hess_coord)
  c  jac_coord_scaled                            iem_jac_coord_scaled
  d  jac_hess_coord + scatter_reduce(amax)       today's row maxima at the start point (_Scaled.__init__)
  e  jac_row_maxabs                              iem_jac_rowmax
  f  cons + c.mul_(s)                            today's scaled constraints
  g  cons_scaled                                 iem_cons_scaled

Per case one child process under its own `timeout` (the parent never opens the GPU and stops at the first child that fails):
every sequence is checked against its counterpart (b = c, d = e, f = g, bitwise), warmed, then timed in blocks of back-to-back
repetitions between one event pair, the sequences taking turns, `--repeats` blocks each; median, minimum and maximum per
repetition.  The bytes are the generator's own account (iem_kernel_info: alg_bytes_read / alg_bytes_written of the kernels a
sequence launches; the torch passes of b, d and f are not in them but are in the time).

  python tools/scaled_bench.py --out profiles/scaled.json
  python tools/scaled_bench.py --case quadrotor_100000          (one case, JSON on stdout)
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"quadrotor_100000": 100_000, "quadrotor_1000000": 1_000_000}
SEQS = ("a jac_coord", "b jac_coord+mul_(s[rows])", "c jac_coord_scaled", "d jac_hess_coord+scatter_reduce(amax)", "e jac_row_maxabs",
        "f cons+mul_(s)", "g cons_scaled")


def one(case, launches, repeats):
    import numpy as np
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib, transcribe, workloads
    from infiniteexamodels.jl_amd.model import ExaModel
    gm = ExaModel(transcribe.exa_core(workloads.quadrotor(CASES[case])), device=0)
    n, mc, nj, nh = gm.meta.nvar, gm.meta.ncon, gm.meta.nnzj, gm.meta.nnzh
    rng = np.random.default_rng(0)
    xd = torch.tensor(gm.meta.x0 + 0.1 * rng.standard_normal(n), device="cuda")
    sd = torch.tensor(np.exp2(rng.uniform(-3.0, 3.0, mc)), device="cuda")
    y0 = torch.zeros(mc, dtype=torch.float64, device="cuda")
    rows = gm.jac_structure_device(0)[0]
    new = lambda k: torch.empty(max(k, 1), dtype=torch.float64, device="cuda")
    jv, jv2, hv, c, c2, rm = new(nj), new(nj), new(nh), new(mc), new(mc), new(mc)
    out = {}
    p = lambda a: C.c_void_p(a.data_ptr())
    L, h = gm._L, gm._h
    gm.scaled_prepare()
    gm._sync_stream()

    def seq_a():
        iemlib.check(L.iem_jac_coord(h, p(xd), p(jv)))

    def seq_b():
        iemlib.check(L.iem_jac_coord(h, p(xd), p(jv)))
        jv.mul_(sd[rows])

    def seq_c():
        iemlib.check(L.iem_jac_coord_scaled(h, p(xd), p(sd), p(jv2)))

    def seq_d():
        iemlib.check(L.iem_jac_hess_coord(h, p(xd), p(y0), 0.0, p(jv), p(hv)))
        out["d"] = torch.zeros(mc, dtype=torch.float64, device="cuda").scatter_reduce(0, rows, jv.abs(), reduce="amax")

    def seq_e():
        iemlib.check(L.iem_jac_rowmax(h, p(xd), p(rm)))

    def seq_f():
        iemlib.check(L.iem_cons(h, p(xd), p(c)))
        c.mul_(sd)

    def seq_g():
        iemlib.check(L.iem_cons_scaled(h, p(xd), p(sd), p(c2)))

    seqs = dict(zip(SEQS, (seq_a, seq_b, seq_c, seq_d, seq_e, seq_f, seq_g)))
    # the pairs agree bitwise before anything is timed
    seq_b(); seq_c(); seq_d(); seq_e(); seq_f(); seq_g(); torch.cuda.synchronize()
    assert torch.equal(jv2.view(torch.int64), (sd[rows] * gm.jac_coord(xd)).view(torch.int64)), "jac_coord_scaled is not jac_coord times s[rows]"
    assert torch.equal(rm.view(torch.int64), out["d"].view(torch.int64)), "jac_row_maxabs is not today's row maxima"
    assert torch.equal(c2.view(torch.int64), c.view(torch.int64)), "cons_scaled is not cons times s"
    for s in SEQS:
        for _ in range(20):
            seqs[s]()
    torch.cuda.synchronize()
    us = {s: [] for s in SEQS}
    for _ in range(repeats):
        for s in SEQS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                seqs[s]()
            e1.record(); torch.cuda.synchronize()
            us[s].append(e0.elapsed_time(e1) / launches * 1e3)
    own, mine = gm.kernels(), gm.scaled_kernels()
    kind = lambda ks, k: [q for q in ks if q["kind"] == k]
    launched = dict(zip(SEQS, (kind(own, "jac"), kind(own, "jac"), kind(mine, "jac"), kind(own, "pair") or kind(own, "jac") + kind(own, "hess"),
                               kind(mine, "jprod"), kind(own, "cons"), kind(mine, "cons"))))
    res = {"case": case, "nvar": n, "ncon": mc, "nnzj": nj, "nnzh": nh, "launches_per_block": launches, "repeats": repeats,
           "jit": bool(any(k["jit"] for k in own + mine)), "device": torch.cuda.get_device_name(0), "sequences": {}}
    for s in SEQS:
        ks = launched[s]
        med = float(np.median(us[s]))
        res["sequences"][s] = {"us_median": round(med, 3), "us_min": round(min(us[s]), 3), "us_max": round(max(us[s]), 3),
                               "kernels": [q["name"] for q in ks], "workgroups": [int(np.prod(q["grid"])) for q in ks],
                               "alg_bytes_read": sum(q["alg_bytes_read"] for q in ks), "alg_bytes_written": sum(q["alg_bytes_written"] for q in ks)}
    m = {s[0]: res["sequences"][s]["us_median"] for s in SEQS}
    res["order"] = {"c < b": m["c"] < m["b"], "e < d": m["e"] < m["d"], "g < f": m["g"] < m["f"]}
    gm.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per case (child process)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scaled.json"))
    a = ap.parse_args()
    if a.case:
        print(json.dumps(one(a.case, a.launches, a.repeats)))
        return 0
    doc = {"what": "tools/scaled_bench.py: per-repetition time of the scaled Jacobian, the row maxima and the scaled constraints from the "
                   "scaled kernels and from today's path (the model's kernels plus torch passes), device events around blocks of "
                   "back-to-back repetitions, warm; median / min / max over the blocks, beside the algorithmic bytes iem_kernel_info "
                   "reports for the kernels each sequence launches (the torch passes are in the time, not in the bytes)",
           "cases": []}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for case in a.cases.split(","):
        r = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--case", case,
                            "--launches", str(a.launches), "--repeats", str(a.repeats)], stdout=subprocess.PIPE, text=True)
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
