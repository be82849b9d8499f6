#!/usr/bin/env python3
"""What a solver's convergence check costs: c(x), f(x) and r = σ·∇f(x) + J(x)ᵀ·y, three ways, in the same run on one handle.

  1  eval_residual                      iem_eval_residual: one launch (plus the deterministic follow-ups of lagrad's scatter)
  2  lagrangian_grad + eval_trial       iem_lagrad, then iem_eval_trial — which returns f on the HOST: its round trip is in it
  3  grad + jtprod + cons + obj_device  ... and the torch add  r = Jᵀy + σ·g: the sequence the in-tree solvers run today

Per case one child process under its own `timeout` (the parent never opens the GPU and stops at the first child that fails):
every sequence is warmed, then timed in blocks of back-to-back repetitions between one event pair, alternating the
sequences, `--repeats` blocks each; median, minimum and maximum per repetition.  The bytes are the generator's own account
(iem_kernel_info: alg_bytes_read / alg_bytes_written of the kernels a sequence launches; follow-up launches, memsets and the
torch add are not in them but are in the time).

  python tools/residual_bench.py --out profiles/residual.json
  python tools/residual_bench.py --case quadrotor_100000          (one case, JSON on stdout)
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"quadrotor_1000": ("quadrotor", 1_000), "quadrotor_16000": ("quadrotor", 16_000), "quadrotor_100000": ("quadrotor", 100_000),
         "quadrotor_1000000": ("quadrotor", 1_000_000), "pandemic_110x128": ("pandemic", (110, 128))}
SEQS = ("eval_residual", "lagrangian_grad+eval_trial", "grad+jtprod+cons+obj_device+add")
SIGMA = 0.7


def one(case, launches, repeats):
    import numpy as np
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib, transcribe, workloads
    from infiniteexamodels.jl_amd.model import ExaModel
    wl, size = CASES[case]
    im = workloads.quadrotor(size) if wl == "quadrotor" else workloads.pandemic(size[0], size[1])
    core = transcribe.exa_core(im)
    gm = ExaModel(core, device=0)
    n, mc = gm.meta.nvar, gm.meta.ncon
    rng = np.random.default_rng(0)
    xd = torch.tensor(gm.meta.x0 + 0.1 * rng.standard_normal(n), device="cuda")
    yd = torch.tensor(rng.standard_normal(mc), device="cuda")
    new = lambda k: torch.empty(max(k, 1), dtype=torch.float64, device="cuda")
    r, c, f, g, jt = new(n), new(mc), new(1), new(n), new(n)
    p = lambda a: C.c_void_p(a.data_ptr())
    L, h = gm._L, gm._h
    gm.lagrangian_prepare()
    gm._sync_stream()
    fh = C.c_double()

    def seq1():
        iemlib.check(L.iem_eval_residual(h, p(xd), p(yd), SIGMA, p(c), p(r), p(f)))

    def seq2():
        iemlib.check(L.iem_lagrad(h, p(xd), p(yd), SIGMA, p(r)))
        iemlib.check(L.iem_eval_trial(h, p(xd), p(c), C.byref(fh)))

    def seq3():
        iemlib.check(L.iem_grad(h, p(xd), p(g)))
        iemlib.check(L.iem_jtprod(h, p(xd), p(yd), p(jt)))
        iemlib.check(L.iem_cons(h, p(xd), p(c)))
        iemlib.check(L.iem_obj_device(h, p(xd), p(f)))
        torch.add(jt, g, alpha=SIGMA, out=r)

    seqs = dict(zip(SEQS, (seq1, seq2, seq3)))
    # the three agree before anything is timed (1 and 2 bitwise; 3 adds in another order)
    seq1(); r1, c1, f1 = r.clone(), c.clone(), float(f.item())
    seq2(); torch.cuda.synchronize()
    assert torch.equal(r, r1) and torch.equal(c, c1) and fh.value == f1, "eval_residual and lagrangian_grad + eval_trial disagree"
    seq3(); torch.cuda.synchronize()
    scale = max(1.0, float(r1.abs().max()))
    assert float((r - r1).abs().max()) <= 1e-10 * scale and torch.equal(c, c1) and float(f.item()) == f1, "today's sequence disagrees"
    for s in SEQS:
        for _ in range(30):
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
    own, mine = gm.kernels(), gm.lagrangian_kernels()
    pick = lambda ks, names: [q for q in ks if q["name"] in names]
    phase = pick(mine, ("iem_residual_all",))
    members = pick(mine, ("iem_cons_all", "iem_obj_all", "iem_lagrad_all")) + [q for q in mine if q["name"].startswith(("iem_cons_g", "iem_lagrad_g"))]
    launched = {SEQS[0]: phase or members,
                SEQS[1]: [q for q in mine if q["name"].startswith("iem_lagrad")] + ([q for q in own if q["kind"] == "trial"] or [q for q in own if q["kind"] in ("cons", "obj")]),
                SEQS[2]: [q for q in own if q["kind"] in ("grad", "jtprod", "cons", "obj")]}
    res = {"case": case, "nvar": n, "ncon": mc, "launches_per_block": launches, "repeats": repeats, "one_launch": bool(phase),
           "jit": bool(any(k["jit"] for k in own + mine)), "device": torch.cuda.get_device_name(0), "sequences": {}}
    for s in SEQS:
        ks = launched[s]
        rb, wb = sum(q["alg_bytes_read"] for q in ks), sum(q["alg_bytes_written"] for q in ks)
        med = float(np.median(us[s]))
        res["sequences"][s] = {"us_median": round(med, 3), "us_min": round(min(us[s]), 3), "us_max": round(max(us[s]), 3),
                               "kernels": [q["name"] for q in ks], "workgroups": [int(np.prod(q["grid"])) for q in ks],
                               "alg_bytes_read": rb, "alg_bytes_written": wb}
    gm.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--timeout", type=int, default=400, help="seconds per case (child process)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "residual.json"))
    a = ap.parse_args()
    if a.case:
        print(json.dumps(one(a.case, a.launches, a.repeats)))
        return 0
    doc = {"what": "tools/residual_bench.py: per-repetition time of a convergence check (c, f, σ∇f + Jᵀy) as one launch, as lagrangian_grad + "
                   "eval_trial (f returned on the host) and as today's grad + jtprod + cons + obj_device + torch add (device events around "
                   "blocks of back-to-back repetitions, warm; median / min / max over the blocks) beside the algorithmic bytes "
                   "iem_kernel_info reports for the kernels each sequence launches",
           "cases": []}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for case in a.cases.split(","):
        r = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--case", case,
                            "--launches", str(a.launches), "--repeats", str(a.repeats)], stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            print(f"{case}: FAILED with exit status {r.returncode}; nothing more is started", file=sys.stderr)
            return 1
        doc["cases"].append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(case, {k: v["us_median"] for k, v in doc["cases"][-1]["sequences"].items()}, "us", flush=True)
        with open(a.out, "w") as f:      # after every case: what was measured stays if a later case fails
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
