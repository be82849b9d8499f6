#!/usr/bin/env python3
"""What Mehrotra's corrector on the device (iem_mpc_*) costs per call, beside the first-order calls that move almost the same bytes,
what the whole corrector costs per iteration, and what the same quantities cost by torch expressions with the decision on the host,
measured in the same process.

  barrier_terms, mpc_terms                        µs per call on the same state (mpc_terms writes two columns and reads the six affine
                                                  vectors; it writes neither sigma nor dcon)
  barrier_step, mpc_step                          µs per call on the same state and solution
  amu_probe                                       the safeguard's measurement
  select_taken, select_refused                    iem_mpc_select with a probe that lets the corrector through (the copy) and one that
                                                  does not (a few words)
  solve_1, solve_2                                iem_kkt_solve_refined_diag (one refinement step) with one and with two columns on the
                                                  same factors: the second column is solve_2 − solve_1
  corrector                                       per iteration: mpc_terms − barrier_terms + (solve_2 − solve_1) + mpc_step + amu_probe +
                                                  select_taken, from the medians above — and `corrector_sequence`: mpc_terms, the
                                                  two-column solve, barrier_step, mpc_step, amu_probe, select back to back (device
                                                  events), beside `first_order_sequence`: barrier_terms, the one-column solve, barrier_step
  torch                                           the second column's right-hand side, the corrected directions, the two step lengths,
                                                  the probe and the decision by torch expressions over the full vectors (masks for
                                                  the present bounds) with ONE read-back and the decision on the host, then the copy
                                                  (wall clock; no solve) — beside `device_no_solve`: mpc_terms + mpc_step + amu_probe +
                                                  select + iem_mpc_state, wall clock

The sizes and the method of tools/qf_bench.py: per case one child process under its own `timeout` (the parent never opens the GPU and
stops at the first child that fails); every sequence warmed, then blocks of back-to-back calls between ONE event pair (the sequences
with a read-back: wall clock around the block), `--repeats` blocks each, the sequences taking turns; median, minimum and maximum per
call over the blocks.  No duration existed before this tool: it reports and sets no threshold.

  python tools/mpc_bench.py --out profiles/mpc.json
  python tools/mpc_bench.py --case opf_10000          (one case, JSON on stdout)
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ("pandemic_110_128", "opf_10000", "quadrotor_16000", "quadrotor_100000")
MODELS = {"pandemic_110_128": "workloads.pandemic(110, 128)", "opf_10000": "workloads.opf(10000)", "quadrotor_16000": "workloads.quadrotor(16000)",
          "quadrotor_100000": "workloads.quadrotor(100000)"}
MU, TAU, RELAX, DW, DC = 0.1, 0.99, 1e-8, 1e-2, 1e-6


def one(case, block, repeats):
    import ctypes as C
    import numpy as np
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib, transcribe, workloads
    from infiniteexamodels.jl_amd.barrier import AdaptiveBarrierParameter, BarrierLayer, BarrierParameter, MehrotraCorrector
    from infiniteexamodels.jl_amd.kkt_chain import KKTObject
    from infiniteexamodels.jl_amd.model import ExaModel
    gm = ExaModel(transcribe.exa_core(eval(MODELS[case], {"workloads": workloads})), device=0)
    meta = gm.meta
    n, m = int(meta.nvar), int(meta.ncon)
    lvar, uvar, lcon, ucon = (np.asarray(a, dtype=np.float64) for a in (meta.lvar, meta.uvar, meta.lcon, meta.ucon))
    parts, fx, fc, info = iemlib.barrier_analyse(lvar, uvar, lcon, ucon, RELAX)
    rng = np.random.default_rng(0)
    hasL, hasU, gL, gU = (fx & 1) > 0, (fx & 2) > 0, (fc & 1) > 0, (fc & 2) > 0

    def inside(v, lo, hi, a, b):
        with np.errstate(invalid="ignore"):
            v = np.where(a & b, lo + rng.uniform(0.05, 0.95, len(v)) * (hi - lo), v)
            v = np.where(a & ~b, lo + 10.0 ** rng.uniform(-2, 1, len(v)), v)
            return np.where(b & ~a, hi - 10.0 ** rng.uniform(-2, 1, len(v)), v)
    x = inside(np.asarray(meta.x0, dtype=np.float64) + 0.1 * rng.standard_normal(n), parts["xl"], parts["xu"], hasL, hasU)
    T = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")
    new = lambda k: torch.empty(k, dtype=torch.float64, device="cuda")
    xd, yd = T(x), T(0.1 * rng.standard_normal(m))
    _, cd, rd = gm.eval_residual(xd, yd)
    s = inside(cd.cpu().numpy(), parts["rl"], parts["ru"], gL, gU)
    mult = lambda k: T(10.0 ** rng.uniform(-2, 2, k))
    state = (xd, T(s), yd, mult(n), mult(n), mult(m), mult(m))
    small = lambda k: T(1e-3 * rng.standard_normal(k))
    sol_a, dirs_a = small(n + m), (small(m), small(n), small(n), small(m), small(m))
    nz, mi = info["nz"], info["n_ineq"]
    with_x, with_s = int((hasL | hasU).sum()), int((gL | gU).sum())
    # algorithmic bytes, counted as for the sibling kernels: flags, then 8-byte words per entry and per present bound
    b_read = (n + m) + 8 * (n + with_x + m + info["n_eq"] + 2 * mi + 2 * nz)      # flags; r; x; c; ceq | s, y; bound and multiplier per present bound
    b_affine = 8 * (with_x + with_s + nz)                                        # d_aff per entry with a bound, dz_aff per present bound
    b_terms = b_read + 8 * 2 * (n + m)                                           # writes rhs, sigma, dcon
    b_mpc_terms = b_read + b_affine + 8 * 2 * (n + m)                            # writes the two columns
    b_step = (n + m) + 8 * ((n + m) + n + 2 * mi + 2 * nz + 2 * n + 3 * mi)      # flags; sol; x; s, y; bound and multiplier per present bound; the five directions
    b_mpc_step = b_step + b_affine
    b_select = 8 * 5 + 2 * 8 * ((n + m) + 2 * n + 3 * mi) + m                    # the words; taken: six vectors read and written, fc
    res = {"case": case, "model": MODELS[case], "device": torch.cuda.get_device_name(0), "repeats": repeats, "calls_per_block": block, **info,
           "bytes": {"barrier_terms": b_terms, "mpc_terms": b_mpc_terms, "barrier_step": b_step, "mpc_step": b_mpc_step, "select_taken": b_select,
                     "terms_ratio": b_mpc_terms / b_terms, "step_ratio": b_mpc_step / b_step}}

    with BarrierLayer(gm, relax=RELAX) as bar, KKTObject(gm) as kkt, BarrierParameter(bar, mu_init=MU) as par, AdaptiveBarrierParameter(par) as amu, \
            MehrotraCorrector(amu) as mpc:
        sigma, dcon, rhs = bar.terms(state, rd, cd, MU)
        jv, hv = new(int(meta.nnzj)), new(int(meta.nnzh))
        gm.jac_hess_coord(xd, yd, jv, hv, obj_weight=1.0)
        kkt.set_border(1)      # a dense border stays on the device: the solve synchronises nowhere
        kkt.assemble(hv, jv, sigma, DW, DC, dcon=dcon, at=(xd, yd, 1.0))
        res["inertia"] = list(kkt.factor())
        L, k = kkt._handle()
        p = lambda t: C.c_void_p(t.data_ptr())
        rhs2, sol2 = torch.zeros((2, n + m), dtype=torch.float64, device="cuda"), torch.zeros((2, n + m), dtype=torch.float64, device="cuda")

        def solve(nrhs):      # one refinement step, buffers of the caller: no allocation
            kkt._handle()
            iemlib.check(L.iem_kkt_solve_refined_diag(k, p(xd), p(yd), 1.0, p(sigma), p(dcon), DW, DC, nrhs, p(rhs2), n + m, p(sol2), n + m, 1, None))
        mk = lambda: (torch.zeros(m, dtype=torch.float64, device="cuda"), new(n), new(n), torch.zeros(m, dtype=torch.float64, device="cuda"),
                      torch.zeros(m, dtype=torch.float64, device="cuda"))
        dirs, dirs_c, alpha, alpha_c, q_c = mk(), mk(), new(2), new(2), new(4)
        mpc.terms(state, rd, cd, sol_a, dirs_a, MU, out=rhs2)
        solve(2)
        mpc.step(state, sol_a, dirs_a, sol2[1], MU, TAU, out=dirs_c, alpha=alpha_c)
        amu.probe(state, sol2[1], dirs_c, alpha_c, out=q_c)
        torch.cuda.synchronize()
        rt = C.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))
        rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        ab = np.zeros(16)
        assert rt.hipMemcpy(ab.ctypes.data, amu.device(), 128, 2) == 0
        ab[9] = 1.0      # avg: the decision is then in the probe's hands
        assert rt.hipMemcpy(amu.device(), ab.ctypes.data, 128, 1) == 0
        q_take, q_refuse, a_ok = T([0.5 * max(nz, 1), 0.0, 0.5, 0.5]), T([2.0 * max(nz, 1), 0.0, 0.5, 0.5]), T([0.5, 0.5])
        res["alpha_c"], res["probe_c"] = alpha_c.tolist(), q_c.tolist()
        bd = {key: T(np.where(np.isfinite(parts[key]), parts[key], 0.0)) for key in ("xl", "xu", "rl", "ru")}
        on = {key: torch.tensor(v, device="cuda") for key, v in (("xL", hasL), ("xU", hasU), ("sL", gL), ("sU", gU))}
        one_n, one_m = torch.ones(n, dtype=torch.float64, device="cuda"), torch.ones(m, dtype=torch.float64, device="cuda")
        zero_n, zero_m = torch.zeros_like(one_n), torch.zeros_like(one_m)
        ine = on["sL"] | on["sU"]

        def by_torch():
            xs, ss, ys, zL, zU, vL, vU = state
            dxa, (dsa, dzLa, dzUa, dvLa, dvUa) = sol_a[:n], dirs_a
            gxl, gxu, gsl, gsu = xs - bd["xl"], bd["xu"] - xs, ss - bd["rl"], bd["ru"] - ss
            ml = torch.where(on["xL"], (MU - dxa * dzLa) / gxl, zero_n); mu_u = torch.where(on["xU"], (MU + dxa * dzUa) / gxu, zero_n)
            nl = torch.where(on["sL"], (MU - dsa * dvLa) / gsl, zero_m); nu = torch.where(on["sU"], (MU + dsa * dvUa) / gsu, zero_m)
            tl, tu = torch.where(on["sL"], vL / gsl, zero_m), torch.where(on["sU"], vU / gsu, zero_m)
            sigs = tl + tu
            rs = (nu - nl) - ys
            col1 = torch.cat([-(rd + (mu_u - ml)), torch.where(ine, -((cd - ss) + rs / sigs), -cd)])      # the second column (equality rows: ceq taken as 0)
            dx, dy = sol2[1][:n], sol2[1][n:]
            ds = torch.where(ine, (dy - rs) / sigs, zero_m)
            dzL = torch.where(on["xL"], (ml - zL) - (zL / gxl) * dx, zero_n); dzU = torch.where(on["xU"], (mu_u - zU) + (zU / gxu) * dx, zero_n)
            dvL = torch.where(on["sL"], (nl - vL) - tl * ds, zero_m); dvU = torch.where(on["sU"], (nu - vU) + tu * ds, zero_m)
            cand = lambda num, den, mask: torch.where(mask, num / den, one_n if len(den) == n else one_m).clamp(max=1.0).min()
            ap = torch.minimum(torch.minimum(cand(-TAU * gxl, dx, on["xL"] & (dx < 0)), cand(TAU * gxu, dx, on["xU"] & (dx > 0))),
                               torch.minimum(cand(-TAU * gsl, ds, on["sL"] & (ds < 0)), cand(TAU * gsu, ds, on["sU"] & (ds > 0))))
            ad = torch.minimum(torch.minimum(cand(-TAU * zL, dzL, on["xL"] & (dzL < 0)), cand(-TAU * zU, dzU, on["xU"] & (dzU < 0))),
                               torch.minimum(cand(-TAU * vL, dvL, on["sL"] & (dvL < 0)), cand(-TAU * vU, dvU, on["sU"] & (dvU < 0))))
            tx, ts = ap * dx, ap * ds
            pr = torch.cat([torch.where(on["xL"], (gxl + tx) * (zL + ad * dzL), zero_n), torch.where(on["xU"], (gxu - tx) * (zU + ad * dzU), zero_n),
                            torch.where(on["sL"], (gsl + ts) * (vL + ad * dvL), zero_m), torch.where(on["sU"], (gsu - ts) * (vU + ad * dvU), zero_m)])
            total, bad, a_p, a_d = torch.stack([pr.sum(), torch.isnan(pr).sum().to(torch.float64), ap, ad]).tolist()      # THE read-back
            taken = nz != 0 and bad == 0 and a_p != 0.0 and a_d != 0.0 and total / max(nz, 1) <= 1e300      # (always taken where there is a bound: the copy is timed)
            if taken:
                sol2[0].copy_(sol2[1])
                for dst, src in zip(dirs, (ds, dzL, dzU, dvL, dvU)):
                    dst.copy_(src)
                alpha.copy_(torch.stack([ap, ad]))
            return col1, taken

        def device_no_solve():
            mpc.terms(state, rd, cd, sol_a, dirs_a, MU, out=rhs2)
            mpc.step(state, sol_a, dirs_a, sol2[1], MU, TAU, out=dirs_c, alpha=alpha_c)
            amu.probe(state, sol2[1], dirs_c, alpha_c, out=q_c)
            mpc.select(q_take, a_ok, sol2[1], dirs_c, sol2[0], dirs, alpha)
            return mpc.state()

        def corrector_sequence():
            mpc.terms(state, rd, cd, sol_a, dirs_a, MU, out=rhs2)
            solve(2)
            bar.step(state, sol2[0], MU, TAU, out=dirs, alpha=alpha)
            mpc.step(state, sol_a, dirs_a, sol2[1], MU, TAU, out=dirs_c, alpha=alpha_c)
            amu.probe(state, sol2[1], dirs_c, alpha_c, out=q_c)
            mpc.select(q_c, alpha_c, sol2[1], dirs_c, sol2[0], dirs, alpha)

        def first_order_sequence():
            bar.terms(state, rd, cd, MU, out=(sigma, dcon, rhs2[0]))
            solve(1)
            bar.step(state, sol2[0], MU, TAU, out=dirs, alpha=alpha)
        calls = {"barrier_terms": lambda: bar.terms(state, rd, cd, MU, out=(sigma, dcon, rhs)), "mpc_terms": lambda: mpc.terms(state, rd, cd, sol_a, dirs_a, MU, out=rhs2),
                 "barrier_step": lambda: bar.step(state, sol2[1], MU, TAU, out=dirs, alpha=alpha),
                 "mpc_step": lambda: mpc.step(state, sol_a, dirs_a, sol2[1], MU, TAU, out=dirs_c, alpha=alpha_c),
                 "amu_probe": lambda: amu.probe(state, sol2[1], dirs_c, alpha_c, out=q_c),
                 "select_taken": lambda: mpc.select(q_take, a_ok, sol2[1], dirs_c, sol2[0], dirs, alpha),
                 "select_refused": lambda: mpc.select(q_refuse, a_ok, sol2[1], dirs_c, sol2[0], dirs, alpha),
                 "solve_1": lambda: solve(1), "solve_2": lambda: solve(2), "corrector_sequence": corrector_sequence, "first_order_sequence": first_order_sequence,
                 "device_no_solve": device_no_solve, "torch": by_torch}

        def timed(names, blk, wall):
            for nm in names:
                for _ in range(3):
                    calls[nm]()
            torch.cuda.synchronize()
            us = {nm: [] for nm in names}
            for _ in range(repeats):
                for nm in names:
                    torch.cuda.synchronize()
                    if wall:
                        t0 = time.perf_counter()
                        for _ in range(blk):
                            calls[nm]()
                        torch.cuda.synchronize()
                        us[nm].append(1e6 * (time.perf_counter() - t0) / blk)
                    else:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(blk):
                            calls[nm]()
                        e1.record(); torch.cuda.synchronize()
                        us[nm].append(1e3 * e0.elapsed_time(e1) / blk)
            return {nm: {"us_median": float(np.median(v)), "us_min": min(v), "us_max": max(v)} for nm, v in us.items()}
        state_taken = device_no_solve()
        assert state_taken["taken"] == (nz != 0), state_taken
        res["us_per_call"] = timed(["barrier_terms", "mpc_terms", "barrier_step", "mpc_step", "amu_probe", "select_taken", "select_refused"], block, wall=False)
        res["us_per_call"].update(timed(["solve_1", "solve_2", "first_order_sequence", "corrector_sequence"], max(2, block // 10), wall=False))
        u = {key: v["us_median"] for key, v in res["us_per_call"].items()}
        res["terms_ratio"], res["step_ratio"] = u["mpc_terms"] / u["barrier_terms"], u["mpc_step"] / u["barrier_step"]
        res["second_column_us"] = u["solve_2"] - u["solve_1"]
        res["corrector_us_per_iteration"] = (u["mpc_terms"] - u["barrier_terms"]) + res["second_column_us"] + u["mpc_step"] + u["amu_probe"] + u["select_taken"]
        res["corrector_sequence_minus_first_order_us"] = u["corrector_sequence"] - u["first_order_sequence"]
        res["us_wall_clock_no_solve"] = timed(["device_no_solve", "torch"], max(2, block // 10), wall=True)
        w = res["us_wall_clock_no_solve"]
        res["torch_over_device_no_solve"] = w["torch"]["us_median"] / w["device_no_solve"]["us_median"]
    gm.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=CASES)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--block", type=int, default=100, help="calls between one event pair (a tenth of it for the sequences with a solve or a read-back)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per case (child process)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mpc.json"))
    a = ap.parse_args()
    if a.case:
        print(json.dumps(one(a.case, a.block, a.repeats)))
        return 0
    doc = {"what": "tools/mpc_bench.py: µs per call of iem_mpc_terms beside iem_barrier_terms, iem_mpc_step beside iem_barrier_step, iem_amu_probe, iem_mpc_select taken and "
                   "refused, iem_kkt_solve_refined_diag with one and two columns — device events around blocks of back-to-back calls — with the algorithmic bytes; the "
                   "corrector per iteration from those medians and as one sequence beside the first-order sequence; and terms + step + probe + select + iem_mpc_state "
                   "against the same quantities by torch expressions with one read-back and the decision on the host (wall clock); warm, the sequences taking turns; "
                   "median / min / max over the blocks",
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
        print(case, {q: round(v["us_median"], 2) for q, v in {**c["us_per_call"], **c["us_wall_clock_no_solve"]}.items()}, "us", flush=True)
        with open(a.out, "w") as f:      # after every case: what was measured stays if a later case fails
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
