#!/usr/bin/env python3
"""What the interior-point barrier layer (iem_barrier_*) costs per call, against the same quantities formed by the torch expressions
of contrib/ipm.py (kept here as the baseline, with and without its `.item()` reads).

  start, terms, step, update, error, merit        µs per call of each of the six calls
  set                                             terms + step + update + error: what one iteration adds between evaluation and solver
  torch                                           the same four quantities by element-wise torch launches, every scalar left on the device
  torch+item                                      ... with the host reads of contrib/ipm.py (step lengths, error maxima and sums)

The state is strictly interior (two-sided entries at lo + U(0.05, 0.95)·(hi − lo), one-sided ones 10^U(−2, 1) off their bound), the
direction is N(0, 1)·1e-5 so that `update` keeps it interior over a block; `update` runs on copies restored between blocks.  Per case
one child process under its own `timeout` (the parent never opens the GPU and stops at the first child that fails).  Every sequence
warmed, then blocks of back-to-back calls between ONE event pair, `--repeats` blocks each, the sequences taking turns; median, minimum
and maximum per call over the blocks.  Algorithmic bytes per call (counted from the sizes) are reported beside them.

  python tools/barrier_bench.py --out profiles/barrier.json
  python tools/barrier_bench.py --case opf_10000          (one case, JSON on stdout)
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ("pandemic_110_128", "opf_10000", "quadrotor_16000", "quadrotor_100000")
MU, TAU, KAPPA, RELAX = 0.1, 0.99, 1e10, 1e-8
TAU_SET = 0.5      # in the sets: a block applies ten updates in a row, and a gap that shrinks to 1 % each time would round onto its bound


def alg_bytes(info):
    """bytes every call has to move, from the sizes alone: doubles read + written (bounds and the flag bytes included)"""
    n, m, mi = info["nvar"], info["ncon"], info["n_ineq"]
    bounds_x, bounds_s = 2 * n * 8 + n, 3 * m * 8 + m
    return {"start": (n + m) * 8 + bounds_x + bounds_s + (3 * n + 3 * mi) * 8,
            "terms": (4 * n + 6 * m) * 8 + bounds_x + bounds_s + (2 * n + 2 * m) * 8,
            "step": (4 * n + 5 * m) * 8 + bounds_x + bounds_s + (2 * n + 3 * mi) * 8,
            "update": (6 * n + 7 * m) * 8 + bounds_x + bounds_s + (3 * n + m + 3 * mi) * 8,
            "error": (4 * n + 5 * m) * 8 + bounds_x + bounds_s + 64,
            "merit": (n + 2 * m) * 8 + bounds_x + bounds_s + 16}


def one(case, block, repeats):
    import numpy as np
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib, transcribe, workloads
    from infiniteexamodels.jl_amd.barrier import BarrierLayer
    from infiniteexamodels.jl_amd.model import ExaModel
    make = {"pandemic_110_128": lambda: workloads.pandemic(110, 128), "opf_10000": lambda: workloads.opf(10_000),
            "quadrotor_16000": lambda: workloads.quadrotor(16_000), "quadrotor_100000": lambda: workloads.quadrotor(100_000)}[case]
    gm = ExaModel(transcribe.exa_core(make()), device=0)
    meta = gm.meta
    n, m = int(meta.nvar), int(meta.ncon)
    lvar, uvar, lcon, ucon = (np.asarray(a, dtype=np.float64) for a in (meta.lvar, meta.uvar, meta.lcon, meta.ucon))
    parts, fx, fc, info = iemlib.barrier_analyse(lvar, uvar, lcon, ucon, RELAX)
    rng = np.random.default_rng(0)
    hasL, hasU, gL, gU, eq = (fx & 1) > 0, (fx & 2) > 0, (fc & 1) > 0, (fc & 2) > 0, (fc & 4) > 0

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
    state0 = (xd, T(s), yd, mult(n), mult(n), mult(m), mult(m))
    sol = T(1e-5 * rng.standard_normal(n + m))
    res = {"case": case, "model": {"pandemic_110_128": "workloads.pandemic(110, 128)", "opf_10000": "workloads.opf(10000)", "quadrotor_16000": "workloads.quadrotor(16000)", "quadrotor_100000": "workloads.quadrotor(100000)"}[case], "device": torch.cuda.get_device_name(0), "repeats": repeats, "calls_per_block": block, **info}

    with BarrierLayer(gm, relax=RELAX) as bar:
        state = tuple(t.clone() for t in state0)
        tb = (gm._new(n), gm._new(m), gm._new(n + m))
        dirs, alpha = bar.step(state, sol, MU, TAU)
        alpha_first = alpha.tolist()
        alpha_small = alpha * 1e-3      # for the hundred back-to-back updates of a block: the state stays inside its bounds
        alpha_set = gm._new(2)
        out8, out2 = gm._new(8), gm._new(2)
        xs, outs = xd.clone(), tuple(gm._new(k) for k in (m, n, n, m, m))

        def restore():
            for a, b in zip(state, state0):
                a.copy_(b)
        calls = {"start": lambda: bar.start(xs, cd, y=yd, out=outs), "terms": lambda: bar.terms(state, rd, cd, MU, out=tb),
                 "step": lambda: bar.step(state, sol, MU, TAU, out=dirs, alpha=alpha), "update": lambda: bar.update(state, sol, dirs, alpha_small, MU, KAPPA),
                 "error": lambda: bar.error(state, rd, cd, MU, out=out8), "merit": lambda: bar.merit(state[0], state[1], cd, out=out2)}
        calls["set"] = lambda: (calls["terms"](), bar.step(state, sol, MU, TAU_SET, out=dirs, alpha=alpha_set), bar.update(state, sol, dirs, alpha_set, MU, KAPPA),
                                calls["error"]())

        # ---- the baseline: contrib/ipm.py's expressions on compacted inequality rows ------------------------------------
        xl, xu = T(parts["xl"]), T(parts["xu"])
        ine = np.nonzero(~eq)[0]
        ine_idx = torch.as_tensor(ine, device="cuda")
        sl, su = T(parts["rl"][ine]), T(parts["ru"][ine])
        Lx, Ux, Ls, Us = torch.isfinite(xl), torch.isfinite(xu), torch.isfinite(sl), torch.isfinite(su)
        ceq = T(parts["ceq"])
        big, bigs = torch.full_like(xl, float("inf")), torch.full_like(sl, float("inf"))
        Z = lambda on, v: torch.where(on, v, torch.zeros_like(v))
        base0 = (state0[0], state0[1][ine_idx], state0[2], Z(Lx, state0[3]), Z(Ux, state0[4]), Z(Ls, state0[5][ine_idx]), Z(Us, state0[6][ine_idx]))
        base = [t.clone() for t in base0]

        def gaps(xx, ss):
            return (torch.where(Lx, xx - xl, big), torch.where(Ux, xu - xx, big), torch.where(Ls, ss - sl, bigs), torch.where(Us, su - ss, bigs))

        def infeasibility(cc, ss):
            r = cc - ceq
            r[ine_idx] = cc[ine_idx] - ss
            return r

        def torch_set(item):
            xx, ss, yy, zL, zU, vL, vU = base
            read = (lambda t: float(t.item())) if item else (lambda t: t)
            dL, dU, eL, eU = gaps(xx, ss)
            sig_x = zL / dL + zU / dU
            sig_s = vL / eL + vU / eU
            gx = rd - Z(Lx, MU / dL) + Z(Ux, MU / dU)
            gs = -Z(Ls, MU / eL) + Z(Us, MU / eU)
            r_s = gs - yy[ine_idx]
            rp = infeasibility(cd, ss)
            dcv = torch.zeros(m, dtype=torch.float64, device="cuda")
            dcv[ine_idx] = 1.0 / sig_s
            rc = rp.clone()
            rc[ine_idx] = rp[ine_idx] + r_s / sig_s
            rhs = -torch.cat([gx, rc])
            dx, dy = sol[:n], sol[n:]
            ds = (dy[ine_idx] - r_s) / sig_s
            one_ = torch.ones((), dtype=torch.float64, device="cuda")

            def ftb(dv, lo, hi):
                if not dv.numel():
                    return 1.0 if item else one_
                inf_ = torch.full_like(dv, float("inf"))
                a = torch.where(dv < 0, -TAU_SET * lo / dv, inf_).min()
                b = torch.where(dv > 0, TAU_SET * hi / dv, inf_).min()
                return min(1.0, read(a), read(b)) if item else torch.minimum(one_, torch.minimum(a, b))
            ap = ftb(dx, dL, dU), ftb(ds, eL, eU)
            ap = min(ap) if item else torch.minimum(*ap)
            dzL = Z(Lx, MU / dL - zL - zL / dL * dx)
            dzU = Z(Ux, MU / dU - zU + zU / dU * dx)
            dvL = Z(Ls, MU / eL - vL - vL / eL * ds)
            dvU = Z(Us, MU / eU - vU + vU / eU * ds)
            ad = 1.0 if item else one_
            for z_, dz_ in ((zL, dzL), (zU, dzU), (vL, dvL), (vU, dvU)):
                if z_.numel():
                    c_ = torch.where(dz_ < 0, -TAU_SET * z_ / dz_, torch.full_like(z_, float("inf"))).min()
                    ad = min(ad, read(c_)) if item else torch.minimum(ad, c_)
            xx, ss, yy = xx + ap * dx, ss + ap * ds, yy + ap * dy
            zL, zU, vL, vU = zL + ad * dzL, zU + ad * dzU, vL + ad * dvL, vU + ad * dvU
            dL, dU, eL, eU = gaps(xx, ss)
            zL = torch.where(Lx, torch.minimum(torch.maximum(zL, MU / (KAPPA * dL)), KAPPA * MU / dL), zL)
            zU = torch.where(Ux, torch.minimum(torch.maximum(zU, MU / (KAPPA * dU)), KAPPA * MU / dU), zU)
            vL = torch.where(Ls, torch.minimum(torch.maximum(vL, MU / (KAPPA * eL)), KAPPA * MU / eL), vL)
            vU = torch.where(Us, torch.minimum(torch.maximum(vU, MU / (KAPPA * eU)), KAPPA * MU / eU), vU)
            base[:] = [xx, ss, yy, zL, zU, vL, vU]
            # errors
            rdual = rd - zL + zU
            rsl = -yy[ine_idx] - vL + vU
            rp = infeasibility(cd, ss)
            comp = torch.cat([(dL * zL - MU)[Lx], (dU * zU - MU)[Ux], (eL * vL - MU)[Ls], (eU * vU - MU)[Us]])
            vals = [rdual.abs().max(), rp.abs().max(), yy.abs().sum(), zL.sum() + zU.sum() + vL.sum() + vU.sum(), rp.abs().sum(),
                    torch.log(dL[Lx]).sum() + torch.log(dU[Ux]).sum() + torch.log(eL[Ls]).sum() + torch.log(eU[Us]).sum()]
            if rsl.numel():
                vals.append(rsl.abs().max())
            if comp.numel():
                vals.append(comp.abs().max())
            return [read(v) for v in vals], sig_x, dcv, rhs

        def restore_base():
            base[:] = [t.clone() for t in base0]
        calls["torch"] = lambda: torch_set(False)
        calls["torch+item"] = lambda: torch_set(True)

        def timed(names, blk):
            for nm in names:
                restore(); restore_base()
                for _ in range(3):
                    calls[nm]()
            torch.cuda.synchronize()
            us = {nm: [] for nm in names}
            for _ in range(repeats):
                for nm in names:
                    restore(); restore_base()
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(blk):
                        calls[nm]()
                    e1.record(); torch.cuda.synchronize()
                    us[nm].append(1e3 * e0.elapsed_time(e1) / blk)
            return {nm: {"us_median": float(np.median(v)), "us_min": min(v), "us_max": max(v)} for nm, v in us.items()}
        res["us_per_call"] = timed(["start", "terms", "step", "update", "error", "merit"], block)
        res["us_per_set"] = timed(["set", "torch", "torch+item"], max(2, block // 10))
        res["alg_bytes_per_call"] = alg_bytes(info)
        res["alpha_at_the_start_state"] = alpha_first
        res["alpha_after_the_last_set"] = alpha_set.tolist()      # (> 0: the sets moved the state to the end)
    gm.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=CASES)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--block", type=int, default=100, help="calls between one event pair (a tenth of it for the sets)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per case (child process)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "barrier.json"))
    a = ap.parse_args()
    if a.case:
        print(json.dumps(one(a.case, a.block, a.repeats)))
        return 0
    doc = {"what": "tools/barrier_bench.py: µs per call of the six iem_barrier_* calls, µs per set (terms + step + update + error) and the same set by the torch "
                   "expressions of contrib/ipm.py without and with its .item() reads; device events around blocks of back-to-back calls, warm, the sequences "
                   "taking turns; median / min / max over the blocks; algorithmic bytes counted from the sizes",
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
        print(case, {q: round(v["us_median"], 2) for q, v in {**c["us_per_call"], **c["us_per_set"]}.items()}, "us", flush=True)
        with open(a.out, "w") as f:      # after every case: what was measured stays if a later case fails
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
