#!/usr/bin/env python3
"""What one launch per solver phase saves a solver that scales its NLP, in the same run on one handle.

Trial point (s∘c and s_f·f, the value collected on the host):
  a   eval_trial + c.mul_(s)                               the unscaled phase kernel and a vector pass
  a'  obj_begin + cons_scaled + obj_end                    the scaled constraint kernel beside the objective
  b   eval_trial_scaled                                    iem_eval_trial_scaled
Accepted point (s_f·∇f, the row-scaled Jacobian, the Hessian of σ·s_f·f + (y∘s)'c):
  c   eval_accepted(x, y*s, σ·s_f) + g.mul_(s_f) + jac.mul_(s[rows])
  c'  grad + g.mul_(s_f), jac_coord_scaled, y*s, hess_coord
  d   eval_accepted_scaled                                 iem_eval_accepted_scaled

Per case one child process under its own `timeout` (the parent never opens the GPU and stops at the first child that fails):
the scaled phases are checked against the composed sequences first (c, jac, hess and f bitwise, g to 1e-10), everything is
warmed, then timed in blocks of back-to-back repetitions between one event pair, the sequences taking turns, `--repeats`
blocks each; median, minimum and maximum per repetition.  The bytes are the generator's own account (iem_kernel_info:
alg_bytes_read / alg_bytes_written of the kernels a sequence launches; the torch passes are in the time, not in the bytes).

  python tools/scaled_phase_bench.py --out profiles/scaled_phases.json
  python tools/scaled_phase_bench.py --case quadrotor_100000          (one case, JSON on stdout)
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"quadrotor_1000": ("quadrotor", (1000,)), "quadrotor_16000": ("quadrotor", (16000,)), "quadrotor_100000": ("quadrotor", (100_000,)),
         "quadrotor_1000000": ("quadrotor", (1_000_000,)), "pandemic_110x128": ("pandemic", (110, 128))}
SEQS = ("a eval_trial+mul_(s)", "a' obj_begin+cons_scaled+obj_end", "b eval_trial_scaled",
        "c eval_accepted(y*s)+mul_(s_f)+mul_(s[rows])", "c' grad+mul_,jac_coord_scaled,y*s,hess_coord", "d eval_accepted_scaled")


def one(case, launches, repeats):
    import numpy as np
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib, transcribe, workloads
    from infiniteexamodels.jl_amd.model import ExaModel
    make, args = CASES[case]
    gm = ExaModel(transcribe.exa_core(getattr(workloads, make)(*args)), device=0)
    n, mc, nj, nh = gm.meta.nvar, gm.meta.ncon, gm.meta.nnzj, gm.meta.nnzh
    rng = np.random.default_rng(0)
    xd = torch.tensor(gm.meta.x0 + 0.1 * rng.standard_normal(n), device="cuda")
    sd = torch.tensor(rng.uniform(0.1, 2.0, mc), device="cuda")
    yd = torch.tensor(rng.standard_normal(mc), device="cuda")
    sf, sigma = 0.3, 0.7
    rows = gm.jac_structure_device(0)[0]
    new = lambda k: torch.empty(max(k, 1), dtype=torch.float64, device="cuda")
    c1, c2, c3 = new(mc), new(mc), new(mc)
    g1, g2, g3, j1, j2, j3, h1, h2, h3 = new(n), new(n), new(n), new(nj), new(nj), new(nj), new(nh), new(nh), new(nh)
    f = {k: C.c_double() for k in "abc"}
    p = lambda a: C.c_void_p(a.data_ptr())
    L, h = gm._L, gm._h
    gm.scaled_prepare()
    gm.scaled_phase_prepare()
    gm._sync_stream()

    def seq_a():
        iemlib.check(L.iem_eval_trial(h, p(xd), p(c1), C.byref(f["a"])))
        c1.mul_(sd)

    def seq_a2():
        iemlib.check(L.iem_obj_begin(h, p(xd)))
        iemlib.check(L.iem_cons_scaled(h, p(xd), p(sd), p(c2)))
        iemlib.check(L.iem_obj_end(h, C.byref(f["b"])))

    def seq_b():
        iemlib.check(L.iem_eval_trial_scaled(h, p(xd), p(sd), sf, p(c3), C.byref(f["c"])))

    def seq_c():
        ys = yd * sd
        iemlib.check(L.iem_eval_accepted(h, p(xd), p(ys), sigma * sf, p(g1), p(j1), p(h1)))
        g1.mul_(sf)
        j1.mul_(sd[rows])

    def seq_c2():
        iemlib.check(L.iem_grad(h, p(xd), p(g2)))
        g2.mul_(sf)
        iemlib.check(L.iem_jac_coord_scaled(h, p(xd), p(sd), p(j2)))
        ys = yd * sd
        iemlib.check(L.iem_hess_coord(h, p(xd), p(ys), sigma * sf, p(h2)))

    def seq_d():
        iemlib.check(L.iem_eval_accepted_scaled(h, p(xd), p(yd), p(sd), sf, sigma, p(g3), p(j3), p(h3)))

    seqs = dict(zip(SEQS, (seq_a, seq_a2, seq_b, seq_c, seq_c2, seq_d)))
    for s in SEQS:
        seqs[s]()
    torch.cuda.synchronize()
    bits = lambda t: t.view(torch.int64)
    assert torch.equal(bits(c3), bits(c1)) and torch.equal(bits(c3), bits(c2)), "the scaled trial phase's c is not cons times s"
    assert f["c"].value == sf * f["a"].value == sf * f["b"].value, "the scaled trial phase's f is not s_f times obj"
    assert torch.equal(bits(j3), bits(j1)) and torch.equal(bits(j3), bits(j2)), "the scaled accepted phase's jac is not jac times s[rows]"
    assert torch.equal(bits(h3), bits(h1)) and torch.equal(bits(h3), bits(h2)), "the scaled accepted phase's hess is not hess_coord(x, y*s)"
    gerr = float((g3 - g1).abs().max() / max(1.0, float(g1.abs().max())))
    assert gerr <= 1e-10, "the scaled accepted phase's gradient"
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
    own, scl, sph = gm.kernels(), gm.scaled_kernels(), gm.scaled_phase_kernels()
    kind = lambda ks, *kk: [q for k in kk for q in ks if q["kind"] == k]
    launched = dict(zip(SEQS, (kind(own, "trial") or kind(own, "obj", "cons"), kind(own, "obj") + kind(scl, "cons"), kind(sph, "trial") or kind(sph, "obj", "cons"),
                               kind(own, "accepted") or kind(own, "grad", "jac", "hess"), kind(own, "grad") + kind(scl, "jac") + kind(own, "hess"),
                               kind(sph, "accepted") or kind(sph, "grad", "jac", "hess"))))
    res = {"case": case, "nvar": n, "ncon": mc, "nnzj": nj, "nnzh": nh, "launches_per_block": launches, "repeats": repeats,
           "jit": bool(any(k["jit"] for k in own + scl + sph)), "device": torch.cuda.get_device_name(0), "grad_rel_err": gerr, "sequences": {}}
    for s in SEQS:
        ks = launched[s]
        med = float(np.median(us[s]))
        res["sequences"][s] = {"us_median": round(med, 3), "us_min": round(min(us[s]), 3), "us_max": round(max(us[s]), 3),
                               "kernels": [q["name"] for q in ks], "workgroups": [int(np.prod(q["grid"])) for q in ks],
                               "alg_bytes_read": sum(q["alg_bytes_read"] for q in ks), "alg_bytes_written": sum(q["alg_bytes_written"] for q in ks)}
    m = {s.split()[0]: res["sequences"][s]["us_median"] for s in SEQS}
    res["order"] = {"b <= min(a, a')": m["b"] <= min(m["a"], m["a'"]), "d <= min(c, c')": m["d"] <= min(m["c"], m["c'"])}
    gm.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per case (child process)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scaled_phases.json"))
    a = ap.parse_args()
    if a.case:
        print(json.dumps(one(a.case, a.launches, a.repeats)))
        return 0
    doc = {"what": "tools/scaled_phase_bench.py: per-repetition time of a scaled solver's trial point and accepted point from the scaled "
                   "phase kernels (b, d) and from the sequences available without them (a, a', c, c': the model's kernels, the scaled "
                   "program's, and torch passes), device events around blocks of back-to-back repetitions, warm; median / min / max over "
                   "the blocks, beside the algorithmic bytes iem_kernel_info reports for the kernels each sequence launches (the torch "
                   "passes are in the time, not in the bytes); the trial sequences collect the objective on the host in every repetition",
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
