#!/usr/bin/env python3
"""What the feasibility restoration phase (iem_resto_*) costs per call and per whole restoration iteration, against the same
iteration done the host's way — torch expressions for the terms, the directions, the step lengths, the merit sums, the slope, the
trial point, the update, the error and the return test, with `.tolist()` reads and the tests in Python (measured in the same process;
the evaluation calls, the assembly, the factorisation and the refined solve are the same device calls on both sides).

  enter, terms, step, merit0, begin, trial, merit1, update, error, check, leave
                                                  µs per call.  `prepare` (enter + step: state ACTIVE, directions in the object) runs once
                                                  in front of every block and is not timed; enter appends to the original filter, which
                                                  holds one entry throughout (the new entry dominates the old one); update runs with
                                                  step lengths of 1e-12 (every store happens, the state stays where it is)
  iteration                                       eval_residual(0) + error + jac_hess_coord(0) + terms + assemble + factor_async + refined
                                                  solve + step + merit(0) + begin + {trial + cons + merit(1) + search_accept(inner)} +
                                                  update (1e-12) + obj_device + cons + barrier_merit + check, eager, nothing synchronises
  host_iteration                                  the same iteration the host's way: five read-backs

The state is strictly interior; the KKT object is assembled with delta_w = 1e-2, delta_c = 1e-6.  Per case one child process under
its own `timeout` (the parent never opens the GPU and stops at the first child that fails).  Every sequence warmed, then blocks of
back-to-back calls between ONE event pair, `--repeats` blocks each, the sequences taking turns; median, minimum and maximum per call
over the blocks.  Algorithmic bytes per call (upper counts from the sizes) are reported beside them.

  python tools/resto_bench.py --out profiles/resto.json
  python tools/resto_bench.py --case opf_10000          (one case, JSON on stdout)
"""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ("pandemic_110_128", "opf_10000", "quadrotor_16000", "quadrotor_100000")
MODELS = {"pandemic_110_128": "workloads.pandemic(110, 128)", "opf_10000": "workloads.opf(10000)", "quadrotor_16000": "workloads.quadrotor(16000)",
          "quadrotor_100000": "workloads.quadrotor(100000)"}
MU, TAU, RELAX, DW, DC, RHO, TINY = 0.1, 0.99, 1e-8, 1e-2, 1e-6, 1000.0, 1e-12


def alg_bytes(info):
    """bytes every call has to move, upper counts from the sizes alone (every bound counted as present)"""
    n, m, mi = info["nvar"], info["ncon"], info["n_ineq"]
    d = lambda rd, wr: {"read": 8 * rd + n + m, "written": 8 * wr}
    return {"enter": d(5 * n + 2 * m + 5 * mi, 4 * n + 5 * m + 4 * mi), "terms": d(8 * n + 7 * m + 7 * mi, 2 * n + 2 * m), "step": d(6 * n + 6 * m + 7 * mi, 2 * n + 4 * m + 3 * mi),
            "merit0": d(5 * n + 4 * m + 5 * mi, 0), "merit1": d(5 * n + 4 * m + 5 * mi, 0), "begin": d(6 * n + 4 * m + 6 * mi, 16), "trial": d(2 * n + 4 * m + 2 * mi, n + 2 * m + mi),
            "update": d(8 * n + 10 * m + 8 * mi, 3 * n + 5 * m + 3 * mi), "error": d(8 * n + 7 * m + 7 * mi, 8), "check": d(4 + 2 * 64, 3), "leave": d(2 * (2 * n + 2 * mi), m)}


def one(case, block, repeats):
    import ctypes as C
    import numpy as np
    import torch
    from infiniteexamodels.jl_amd import lib as iemlib, transcribe, workloads
    from infiniteexamodels.jl_amd.barrier import BarrierLayer, FilterSearch, Restoration
    from infiniteexamodels.jl_amd.kkt_chain import KKTObject
    from infiniteexamodels.jl_amd.model import ExaModel
    gm = ExaModel(transcribe.exa_core(eval(MODELS[case], {"workloads": workloads})), device=0)
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
    new = lambda k: torch.empty(k, dtype=torch.float64, device="cuda")
    zeros = lambda k: torch.zeros(k, dtype=torch.float64, device="cuda")
    xd, yd = T(x), T(0.1 * rng.standard_normal(m))
    f0, cd, rd = gm.eval_residual(xd, yd)
    s = inside(cd.cpu().numpy(), parts["rl"], parts["ru"], gL, gU)
    mult = lambda k: T(10.0 ** rng.uniform(-2, 2, k))
    state = (xd, T(s), yd, mult(n), mult(n), mult(m), mult(m))
    res = {"case": case, "model": MODELS[case], "device": torch.cuda.get_device_name(0), "repeats": repeats, "calls_per_block": block, **info}

    with BarrierLayer(gm, relax=RELAX) as bar, KKTObject(gm) as kkt, FilterSearch(bar) as fs, Restoration(fs, rho=RHO) as resto:
        inf0 = bar.error(state, rd, cd, MU)
        mu = max(MU, float(inf0[2]))
        zeta = math.sqrt(mu)
        res["mu"], res["zeta"] = mu, zeta
        jv, hv = new(int(meta.nnzj)), new(int(meta.nnzh))
        sigma, dcon, rhs, sol = new(n), new(m), new(n + m), new(n + m)
        dirs, alpha, tiny = (zeros(m), new(n), new(n), zeros(m), zeros(m)), new(2), T([TINY, TINY])
        xt, st, ct, f1, m2, m3, mt3, e8 = new(n), zeros(m), new(m), new(1), new(2), new(3), new(3), new(8)
        inertia = torch.zeros(3, dtype=torch.int64, device="cuda")
        kkt.set_border(1)      # a dense border stays on the device: the solve synchronises nowhere
        L, k = kkt._handle()
        p = lambda t: C.c_void_p(t.data_ptr())

        def factor_and_solve():      # buffers of the caller, no allocation, no synchronisation
            kkt.assemble(hv, jv, sigma, DW, DC, dcon=dcon, at=(xd, yd, 0.0))
            iemlib.check(L.iem_kkt_factor_async(k, p(inertia)))
            iemlib.check(L.iem_kkt_solve_refined_diag(k, p(xd), p(yd), 0.0, p(sigma), p(dcon), DW, DC, 1, p(rhs), n + m, p(sol), n + m, 1, None))

        def iteration():
            gm.eval_residual(xd, yd, 0.0, c=cd, out=rd, obj=f1)
            resto.error(state, rd, cd, mu, zeta, out=e8)
            gm.jac_hess_coord(xd, yd, jv, hv, obj_weight=0.0)
            resto.terms(state, rd, cd, mu, zeta, out=(sigma, dcon, rhs))
            factor_and_solve()
            resto.step(state, sol, mu, TAU, zeta, out=dirs, alpha=alpha)
            resto.merit(0, xd, state[1], cd, zeta, out=m3)
            resto.begin(state, sol, dirs[0], m3, alpha, mu, zeta)
            resto.trial(state, sol, dirs[0], xt, st)
            gm.cons(xt, ct)
            resto.merit(1, xt, st, ct, zeta, out=mt3)
            resto.inner.accept(mt3[0:1], mt3[1:3], mu, alpha)
            resto.update(state, sol, dirs, tiny, mu)
            gm.obj_device(xd, out=f1)
            gm.cons(xd, cd)
            bar.merit(xd, state[1], cd, out=m2)
            resto.check(f1, m2, MU)

        def prepare():
            resto.enter(state, cd, mu)
            resto.step(state, sol, mu, TAU, zeta, out=dirs, alpha=alpha)
        resto.enter(state, cd, mu)
        iteration()
        torch.cuda.synchronize()
        res["inertia"] = inertia.tolist()
        res["inner_status_after_one_rung"] = resto.inner.state()["status_name"]
        calls = {"enter": lambda: resto.enter(state, cd, mu), "terms": lambda: resto.terms(state, rd, cd, mu, zeta, out=(sigma, dcon, rhs)),
                 "step": lambda: resto.step(state, sol, mu, TAU, zeta, out=dirs, alpha=alpha), "merit0": lambda: resto.merit(0, xd, state[1], cd, zeta, out=m3),
                 "begin": lambda: resto.begin(state, sol, dirs[0], m3, alpha, mu, zeta), "trial": lambda: resto.trial(state, sol, dirs[0], xt, st),
                 "merit1": lambda: resto.merit(1, xt, st, ct, zeta, out=mt3), "update": lambda: resto.update(state, sol, dirs, tiny, mu),
                 "error": lambda: resto.error(state, rd, cd, mu, zeta, out=e8), "check": lambda: resto.check(f1, m2, MU), "leave": lambda: resto.leave(state),
                 "iteration": iteration}

        # ---- the baseline: the same iteration by torch expressions, read-backs and the tests in Python ---------------------------------
        ptr = resto.device()
        torch.cuda.synchronize()
        rt = C.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))
        rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        flat = np.empty(12 * m + 2 * n)
        assert rt.hipMemcpy(flat.ctypes.data, ptr["p"], flat.nbytes, 2) == 0
        H = {q: T(flat[i * m:(i + 1) * m]) for i, q in enumerate(("p", "n", "zp", "zn", "dp", "dn", "dzp", "dzn", "pt", "nt", "sR", "ws"))}
        H["xR"], H["wx"] = T(flat[12 * m:12 * m + n]), T(flat[12 * m + n:])
        fin = lambda a: np.where(np.isfinite(a), a, 0.0)
        xl, xu, rl, ru, ceq = T(fin(parts["xl"])), T(fin(parts["xu"])), T(fin(parts["rl"])), T(fin(parts["ru"])), T(parts["ceq"])
        B_ = lambda a: torch.as_tensor(a, device="cuda")
        Lx, Ux, Ls, Us, ine = B_(hasL), B_(hasU), B_(gL), B_(gU), B_(~eq)
        zn_, zm_, one_ = zeros(n), zeros(m), torch.ones(1, dtype=torch.float64, device="cuda")
        hs = dict(filt=[], theta_start=0.0, theta_max=1e4)

        def host_iteration():
            x_, s_, y_, zL_, zU_, vL_, vU_ = state
            P, N, zp, zn = H["p"], H["n"], H["zp"], H["zn"]
            gm.eval_residual(xd, yd, 0.0, c=cd, out=rd, obj=f1)
            inf = torch.where(ine, cd - s_, cd - ceq)
            dL, dU, eL, eU = x_ - xl, xu - x_, s_ - rl, ru - s_
            zw, zs = zeta * H["wx"], zeta * H["ws"]
            rc = (inf - P) + N
            # error: one read-back
            t = rd + zw * (x_ - H["xR"]) - torch.where(Lx, zL_, zn_) + torch.where(Ux, zU_, zn_)
            u = torch.where(ine, zs * (s_ - H["sR"]) - y_ - torch.where(Ls, vL_, zm_) + torch.where(Us, vU_, zm_), zm_)
            comp = torch.stack([torch.where(Lx, dL * zL_ - mu, zn_).abs().max(), torch.where(Ux, dU * zU_ - mu, zn_).abs().max(), torch.where(Ls, eL * vL_ - mu, zm_).abs().max(),
                                torch.where(Us, eU * vU_ - mu, zm_).abs().max(), (P * zp - mu).abs().max(), (N * zn - mu).abs().max()]).max()
            err = torch.stack([t.abs().max(), torch.stack([u.abs().max(), ((RHO - y_) - zp).abs().max(), ((RHO + y_) - zn).abs().max()]).max(), rc.abs().max(), comp,
                               y_.abs().sum(), zp.sum() + zn.sum()]).tolist()
            gm.jac_hess_coord(xd, yd, jv, hv, obj_weight=0.0)
            # terms
            sl, su, ml, mu_u = torch.where(Lx, zL_ / dL, zn_), torch.where(Ux, zU_ / dU, zn_), torch.where(Lx, mu / dL, zn_), torch.where(Ux, mu / dU, zn_)
            tl, tu, nl, nu = torch.where(Ls, vL_ / eL, zm_), torch.where(Us, vU_ / eU, zm_), torch.where(Ls, mu / eL, zm_), torch.where(Us, mu / eU, zm_)
            gx = (mu_u - ml) + zw * (x_ - H["xR"])
            Dp, Dn, ep, en = P / zp, N / zn, (mu - P * (RHO - y_)) / zp, (mu - N * (RHO + y_)) / zn
            tt, D = (rc - ep) + en, Dp + Dn
            sigs1 = torch.where(ine, (tl + tu) + zs, one_)
            gsr = (nu - nl) + zs * (s_ - H["sR"])
            rs1 = gsr - y_
            sigma.copy_((sl + su) + zw)
            dcon.copy_(torch.where(ine, 1.0 / sigs1 + D, D))
            rhs[:n] = -(rd + gx)
            rhs[n:] = torch.where(ine, -(tt + rs1 / sigs1), -tt)
            factor_and_solve()
            # step: directions and the two step lengths, one read-back
            dx, dy = sol[:n], sol[n:]
            ds = torch.where(ine, (dy - rs1) / sigs1, zm_)
            dp, dn, dzp, dzn = ep + Dp * dy, en - Dn * dy, ((RHO - y_) - zp) - dy, ((RHO + y_) - zn) + dy
            dzL, dzU = torch.where(Lx, (ml - zL_) - sl * dx, zn_), torch.where(Ux, (mu_u - zU_) + su * dx, zn_)
            dvL, dvU = torch.where(Ls, (nl - vL_) - tl * ds, zm_), torch.where(Us, (nu - vU_) + tu * ds, zm_)
            frac = lambda gap, d, on: torch.where(on & (d < 0), (-TAU * gap) / d, one_).min()
            ap, ad = torch.stack([torch.stack([frac(dL, dx, Lx), frac(dU, -dx, Ux), frac(eL, ds, Ls), frac(eU, -ds, Us), frac(P, dp, ine | ~ine), frac(N, dn, ine | ~ine)]).min(),
                                  torch.stack([frac(zL_, dzL, Lx), frac(zU_, dzU, Ux), frac(vL_, dvL, Ls), frac(vU_, dvU, Us), frac(zp, dzp, ine | ~ine),
                                               frac(zn, dzn, ine | ~ine)]).min()]).clamp(max=1.0).tolist()

            def merit(x__, s__, c__, p__, n__):
                inf__ = torch.where(ine, c__ - s__, c__ - ceq)
                logs = (torch.where(Lx, x__ - xl, one_).log().sum() + torch.where(Ux, xu - x__, one_).log().sum() + torch.where(Ls, s__ - rl, one_).log().sum() +
                        torch.where(Us, ru - s__, one_).log().sum() + p__.log().sum() + n__.log().sum())
                fr = RHO * (p__ + n__).sum() + (0.5 * zeta) * ((H["wx"] * (x__ - H["xR"]) ** 2).sum() + torch.where(ine, H["ws"] * (s__ - H["sR"]) ** 2, zm_).sum())
                return fr, ((inf__ - p__) + n__).abs().sum(), logs
            # merit at the state and the slope: one read-back
            fr, th, lg = merit(x_, s_, cd, P, N)
            slope = (gx * dx).sum() + torch.where(ine, gsr * ds, zm_).sum() + ((RHO - mu / P) * dp + (RHO - mu / N) * dn).sum()
            fr0, theta0, lg0, slope_h = torch.stack([fr, th, lg, slope]).tolist()
            phi0 = fr0 - mu * lg0
            # one rung: the trial point, its merit (one read-back) and Algorithm A in Python
            xt_ = x_ + ap * dx
            st_ = torch.where(ine, s_ + ap * ds, zm_)
            gm.cons(xt_, ct)
            frt, tht, lgt = torch.stack(list(merit(xt_, st_, ct, P + ap * dp, N + ap * dn))).tolist()
            phi_t = frt - mu * lgt
            ok = math.isfinite(phi_t) and math.isfinite(tht) and tht <= 1e4 * max(1.0, theta0) and not any(tht >= a_ and phi_t >= b_ for a_, b_ in hs["filt"])
            switching = slope_h < 0.0 and theta0 <= 1e-4 * max(1.0, theta0) and ap * (-slope_h) ** 2.3 > theta0 ** 1.1
            accepted = ok and (phi_t <= phi0 + 1e-8 * ap * slope_h + 10.0 * 2.0 ** -52 * abs(phi0) if switching else (tht <= (1.0 - 1e-5) * theta0 or phi_t <= phi0 - 1e-8 * theta0))
            # update with the step lengths of the device iteration
            guard = lambda z, gap: torch.minimum(torch.maximum(z, mu / (1e10 * gap)), (1e10 * mu) / gap)
            x_.add_(TINY * dx)
            y_.add_(TINY * dy)
            s_.copy_(torch.where(ine, s_ + TINY * ds, s_))
            P.add_(TINY * dp)
            N.add_(TINY * dn)
            zL_.copy_(torch.where(Lx, guard(zL_ + TINY * dzL, x_ - xl), zL_))
            zU_.copy_(torch.where(Ux, guard(zU_ + TINY * dzU, xu - x_), zU_))
            vL_.copy_(torch.where(Ls, guard(vL_ + TINY * dvL, s_ - rl), vL_))
            vU_.copy_(torch.where(Us, guard(vU_ + TINY * dvU, ru - s_), vU_))
            zp.copy_(guard(zp + TINY * dzp, P))
            zn.copy_(guard(zn + TINY * dzn, N))
            # the return test: f (a read-back), theta and the log sum (one more), the test in Python
            f_h = gm.obj(xd)
            gm.cons(xd, cd)
            inf = torch.where(ine, cd - s_, cd - ceq)
            logs = (torch.where(Lx, x_ - xl, one_).log().sum() + torch.where(Ux, xu - x_, one_).log().sum() + torch.where(Ls, s_ - rl, one_).log().sum() +
                    torch.where(Us, ru - s_, one_).log().sum())
            theta, lg = torch.stack([inf.abs().sum(), logs]).tolist()
            phi = f_h - MU * lg
            back = math.isfinite(theta) and math.isfinite(phi) and theta <= 0.9 * hs["theta_start"] and theta <= hs["theta_max"] and not any(theta >= a_ and phi >= b_ for a_, b_ in hs["filt"])
            return err, accepted, back
        calls["host_iteration"] = host_iteration

        def timed(names, blk):
            for nm in names:
                prepare()
                for _ in range(3):
                    calls[nm]()
            torch.cuda.synchronize()
            us = {nm: [] for nm in names}
            for _ in range(repeats):
                for nm in names:
                    prepare()
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(blk):
                        calls[nm]()
                    e1.record(); torch.cuda.synchronize()
                    us[nm].append(1e3 * e0.elapsed_time(e1) / blk)
            return {nm: {"us_median": float(np.median(v)), "us_min": min(v), "us_max": max(v)} for nm, v in us.items()}
        res["us_per_call"] = timed(["enter", "terms", "step", "merit0", "begin", "trial", "merit1", "update", "error", "check", "leave"], block)
        res["us_per_iteration"] = timed(["iteration", "host_iteration"], max(2, block // 10))
        res["alg_bytes_per_call"] = alg_bytes(info)
    gm.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=CASES)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--block", type=int, default=100, help="calls between one event pair (a tenth of it for the iterations)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per case (child process)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resto.json"))
    a = ap.parse_args()
    if a.case:
        print(json.dumps(one(a.case, a.block, a.repeats)))
        return 0
    doc = {"what": "tools/resto_bench.py: µs per call of iem_resto_enter / _terms / _step / _merit / _begin / _trial / _update / _error / _check / _leave, µs per whole "
                   "restoration iteration (evaluation, error, terms, assemble, factor, refined solve, step, merit, begin, one rung, update, obj, cons, merit, check) eager, "
                   "and the same iteration by torch expressions, read-backs and the tests in Python; device events around blocks of back-to-back calls, warm, the "
                   "sequences taking turns; median / min / max over the blocks; algorithmic bytes counted from the sizes",
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
        print(case, {q: round(v["us_median"], 2) for q, v in {**c["us_per_call"], **c["us_per_iteration"]}.items()}, "us", flush=True)
        with open(a.out, "w") as f:      # after every case: what was measured stays if a later case fails
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
