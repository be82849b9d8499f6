#!/usr/bin/env python3
"""What the quality-function oracle on the device (iem_qf_*) costs per call, what one whole section costs eager and inside a captured
graph, and what the same quantities cost by torch expressions with their read-backs, measured in the same process.

  qf_begin, qf_alpha, qf_value, qf_update         µs per call on the same state (alpha and value at the first trial sigma: the block is
                                                  put back to the state behind begin in front of every block of calls, by one device
                                                  copy outside the event pair; value moves the section, so a block of value calls is
                                                  `pairs` calls long at most and begin is issued again between blocks)
  section                                         ONE iem_qf_begin + (max_section_steps + 4) x (iem_qf_alpha + iem_qf_value) +
                                                  iem_qf_update + iem_qf_state (the one read-back), eager
  section_graph                                   the same launches captured once, replayed, then iem_qf_state
  torch                                           the same section by torch expressions over the full vectors (masks for the present
                                                  bounds): per evaluation the two step lengths with ONE read-back and the sum of
                                                  squares with ONE read-back, the golden section and the rule on the host

The sizes and the method of tools/amu_bench.py: per case one child process under its own `timeout` (the parent never opens the GPU and
stops at the first child that fails); every sequence warmed, then blocks of back-to-back calls between ONE event pair (the sequences
with a read-back: wall clock around the block), `--repeats` blocks each, the sequences taking turns; median, minimum and maximum per
call over the blocks.  No duration existed before this tool: it reports and sets no threshold.

  python tools/qf_bench.py --out profiles/qf.json
  python tools/qf_bench.py --case opf_10000          (one case, JSON on stdout)
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
MU, RELAX, GOLDEN = 0.1, 1e-8, 0.6180339887498949


def one(case, block, repeats):
    import ctypes as C
    import numpy as np
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib, transcribe, workloads
    from infiniteexamodels.jl_amd.barrier import AdaptiveBarrierParameter, BarrierLayer, BarrierParameter, QualityFunction
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
    xd, yd = T(x), T(0.1 * rng.standard_normal(m))
    _, cd, rd = gm.eval_residual(xd, yd)
    s = inside(cd.cpu().numpy(), parts["rl"], parts["ru"], gL, gU)
    mult = lambda k: T(10.0 ** rng.uniform(-2, 2, k))
    state = (xd, T(s), yd, mult(n), mult(n), mult(m), mult(m))
    col = lambda: (T(1e-3 * rng.standard_normal(n + m)), T(1e-3 * rng.standard_normal(m)), T(1e-3 * rng.standard_normal(n)), T(1e-3 * rng.standard_normal(n)),
                   T(1e-3 * rng.standard_normal(m)), T(1e-3 * rng.standard_normal(m)))
    d0, d1 = col(), col()
    nz = info["nz"]
    # algorithmic bytes per evaluation, counted as for amu_probe: flags, then 8-byte words per entry and per present bound
    with_x, with_s = int((hasL | hasU).sum()), int((gL | gU).sum())
    bytes_begin = (n + m) + 8 * (n + 2 * m + info["n_ineq"] + info["n_eq"] + nz)      # r; c, ceq or s; y on inequality rows; one multiplier per present bound
    bytes_alpha = (n + m) + 8 * (2 * n + 2 * info["n_ineq"] + with_x + with_s + 4 * nz)      # dx, ds twice; x, s; bound, multiplier and two directions per present bound
    bytes_value = (n + m) + 8 * (3 * with_x + 3 * with_s + 4 * nz)      # x or s and its two directions; bound, multiplier and two directions per present bound
    res = {"case": case, "model": MODELS[case], "device": torch.cuda.get_device_name(0), "repeats": repeats, "calls_per_block": block, **info,
           "bytes": {"qf_begin": bytes_begin, "qf_alpha": bytes_alpha, "qf_value": bytes_value, "per_evaluation": bytes_alpha + bytes_value}}

    with BarrierLayer(gm, relax=RELAX) as bar, BarrierParameter(bar, mu_init=MU) as par, AdaptiveBarrierParameter(par) as amu, QualityFunction(amu) as qf:
        pairs = qf.pairs
        res["pairs"] = pairs
        w12 = gm._new(12)
        par.error(state, rd, cd, out=w12)
        qf.begin(state, rd, cd, w12)
        torch.cuda.synchronize()
        rt = C.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))
        rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        opened = torch.empty(32, dtype=torch.float64, device="cuda")
        assert rt.hipMemcpy(opened.data_ptr(), qf.device(), 256, 3) == 0      # the block behind begin, kept on the device
        reopen = lambda: rt.hipMemcpy(qf.device(), opened.data_ptr(), 256, 3)
        bd = {k: T(np.where(np.isfinite(parts[k]), parts[k], 0.0)) for k in ("xl", "xu", "rl", "ru")}
        on = {k: torch.tensor(v, device="cuda") for k, v in (("xL", hasL), ("xU", hasU), ("sL", gL), ("sU", gU))}
        one_n, one_m = torch.ones(n, dtype=torch.float64, device="cuda"), torch.ones(m, dtype=torch.float64, device="cuda")
        zero_n, zero_m = torch.zeros_like(one_n), torch.zeros_like(one_m)
        n_d, n_p = n + info["n_ineq"], m

        def section():
            qf.begin(state, rd, cd, w12)
            qf.section(state, d0, d1)
            qf.update(w12)
            return qf.state()

        def by_torch():
            xs, ss, ys, zL, zU, vL, vU = state
            tau = 0.99
            t = rd
            t = torch.where(on["xL"], t - zL, t); t = torch.where(on["xU"], t + zU, t)
            ine = on["sL"] | on["sU"]
            u = -ys
            u = torch.where(on["sL"], u - vL, u); u = torch.where(on["sU"], u + vU, u)
            inf = cd - torch.where(ine, ss, zero_m)
            D2, P2, w9 = torch.stack([(t * t).sum() + torch.where(ine, u * u, zero_m).sum(), (inf * inf).sum(), w12[9]]).tolist()      # a read-back
            if nz == 0:
                return 1e-11
            avg = w9 / nz
            lo, hi = max(1e-6, 1e-11 / avg), min(100.0, 1e3)
            hi = max(lo, hi)

            def q_at(sigma):
                tt = sigma * avg
                dx, ds, dzL, dzU, dvL, dvU = (a + tt * (b - a) for a, b in zip(d0, d1))
                dx = dx[:n]
                cand = lambda num, den, mask: torch.where(mask, num / den, one_n if len(den) == n else one_m).clamp(max=1.0).min()
                ap = torch.minimum(torch.minimum(cand(-tau * (xs - bd["xl"]), dx, on["xL"] & (dx < 0)), cand(tau * (bd["xu"] - xs), dx, on["xU"] & (dx > 0))),
                                   torch.minimum(cand(-tau * (ss - bd["rl"]), ds, on["sL"] & (ds < 0)), cand(tau * (bd["ru"] - ss), ds, on["sU"] & (ds > 0))))
                ad = torch.minimum(torch.minimum(cand(-tau * zL, dzL, on["xL"] & (dzL < 0)), cand(-tau * zU, dzU, on["xU"] & (dzU < 0))),
                                   torch.minimum(cand(-tau * vL, dvL, on["sL"] & (dvL < 0)), cand(-tau * vU, dvU, on["sU"] & (dvU < 0))))
                a_p, a_d = torch.stack([ap, ad]).tolist()      # a read-back
                tx, ts = a_p * dx, a_p * ds
                p = torch.cat([torch.where(on["xL"], ((xs - bd["xl"]) + tx) * (zL + a_d * dzL), zero_n), torch.where(on["xU"], ((bd["xu"] - xs) - tx) * (zU + a_d * dzU), zero_n),
                               torch.where(on["sL"], ((ss - bd["rl"]) + ts) * (vL + a_d * dvL), zero_m), torch.where(on["sU"], ((bd["ru"] - ss) - ts) * (vU + a_d * dvU), zero_m)])
                c2, bad = torch.stack([(p * p).sum(), torch.isnan(p).sum().to(torch.float64)]).tolist()      # a read-back
                if bad or a_p == 0.0 or a_d == 0.0:
                    return float("inf")
                return (1.0 - a_d) ** 2 * D2 / n_d + ((1.0 - a_p) ** 2 * P2 / n_p if n_p else 0.0) + c2 / nz
            s0 = min(max(1.0, lo), hi)
            best = [(q_at(s0), s0)]
            s1 = max(lo, s0 * 0.99)
            best.append((q_at(s1), s1))
            a, b = (lo, s1) if best[1][0] <= best[0][0] else (s0, hi)
            if b - a > 1e-2 * b:
                c, d = b - GOLDEN * (b - a), a + GOLDEN * (b - a)
                qc, qd = q_at(c), q_at(d)
                best += [(qc, c), (qd, d)]
                for _ in range(pairs - 4):
                    if qc <= qd:
                        b, d, qd = d, c, qc
                        c = b - GOLDEN * (b - a)
                        if b - a <= 1e-2 * b:
                            break
                        qc = q_at(c)
                        best.append((qc, c))
                    else:
                        a, c, qc = c, d, qd
                        d = a + GOLDEN * (b - a)
                        if b - a <= 1e-2 * b:
                            break
                        qd = q_at(d)
                        best.append((qd, d))
            sigma = min(best, key=lambda v: v[0])[1]
            return min(max(sigma * avg, 1e-11), 1e3 * avg)
        st = section()
        mu_t = by_torch()
        assert st["status_name"] == "iterating" and st["section"]["status_name"] == "done", st
        res["section_found"] = {"sigma": st["section"]["sigma"], "q": st["section"]["q"], "evaluations": st["section"]["evaluations"], "mu": st["mu"], "mu_by_torch": mu_t}
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g):
            qf.begin(state, rd, cd, w12)
            qf.section(state, d0, d1)
            qf.update(w12)

        def section_graph():
            g.replay()
            return qf.state()
        calls = {"qf_begin": lambda: qf.begin(state, rd, cd, w12), "qf_alpha": lambda: qf.alpha(state, d0, d1), "qf_value": lambda: qf.value(state, d0, d1),
                 "qf_update": lambda: qf.update(w12), "section": section, "section_graph": section_graph, "torch": by_torch}

        def timed(names, blk, wall, before=None):
            for nm in names:
                for _ in range(3):
                    calls[nm]()
            torch.cuda.synchronize()
            us = {nm: [] for nm in names}
            for _ in range(repeats):
                for nm in names:
                    if before:
                        before()
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
        res["us_per_call"] = {**timed(["qf_begin", "qf_update"], block, wall=False), **timed(["qf_alpha"], block, wall=False, before=reopen),
                              **timed(["qf_value"], 2, wall=False, before=reopen)}      # (two value calls of an open section: the second is the second trial)
        res["us_per_section_wall_clock"] = timed(["section", "section_graph", "torch"], max(2, block // 10), wall=True)
        w = res["us_per_section_wall_clock"]
        res["torch_over_section"] = w["torch"]["us_median"] / w["section"]["us_median"]
        res["torch_over_section_graph"] = w["torch"]["us_median"] / w["section_graph"]["us_median"]
    gm.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=CASES)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--block", type=int, default=100, help="calls between one event pair (a tenth of it for the whole sections)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per case (child process)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qf.json"))
    a = ap.parse_args()
    if a.case:
        print(json.dumps(one(a.case, a.block, a.repeats)))
        return 0
    doc = {"what": "tools/qf_bench.py: µs per call of iem_qf_begin, iem_qf_alpha, iem_qf_value and iem_qf_update — device events around blocks of back-to-back calls — "
                   "with the algorithmic bytes of the three grid kernels, and µs per whole section — wall clock around blocks: begin + (max_section_steps + 4) x "
                   "(alpha + value) + update + iem_qf_state, eager and as one captured graph, against the same section by torch expressions with two read-backs per "
                   "evaluation and the golden section and the rule on the host; warm, the sequences taking turns; median / min / max over the blocks",
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
        print(case, {q: round(v["us_median"], 2) for q, v in {**c["us_per_call"], **c["us_per_section_wall_clock"]}.items()}, "us", flush=True)
        with open(a.out, "w") as f:      # after every case: what was measured stays if a later case fails
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
