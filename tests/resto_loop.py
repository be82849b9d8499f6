"""tests/soc_loop.py's interior-point loop with the feasibility restoration phase — BarrierLayer + kkt_chain.KKTObject + FilterSearch
+ Restoration (the second-order correction is left out: it has its own loop) — TEST INFRASTRUCTURE for tests/test_gpu_resto.py, not
part of the package.  The host keeps what search_loop.py keeps (the monotone mu rule, the delta_w retry, reset() whenever mu
changes) and reads back what it reads; when the delta_w retries end with a FAILED search it enters the restoration phase instead of
giving up, runs restoration iterations (the same host rules, on the restoration's own mu and inner filter) with ONE status read per
iteration until the device says RETURN, and leaves.  `max_restorations = 0`: the loop of search_loop.py.  No scaling, no nested
restoration; a restoration whose inner search fails, or that does not return within `resto_max_iter`, ends the loop as
"restoration failed"."""
import math

import torch

from infiniteexamodels.jl_amd.barrier import BarrierLayer, FilterSearch, Restoration
from infiniteexamodels.jl_amd.kkt_chain import KKTObject

KAPPA_EPS, KAPPA_MU, THETA_MU, TAU_MIN, DELTA_C = 10.0, 0.2, 1.5, 0.99, 1e-10


def solve(model, x0=None, tol=1e-8, max_iter=200, mu=0.1, rungs=4, refine=1, max_restorations=5, resto_max_iter=100, log=None, resto_opts=None, **search_opts):
    """``dict(status, x, state, objective, iterations, error, statuses, failed, rungs_run, trials, restorations, resto_iterations,
    why)``; status: "solved" | "max_iter" | "search failed" | "restoration failed" """
    n, m = int(model.meta.nvar), int(model.meta.ncon)
    new = lambda k: torch.empty(k, dtype=torch.float64, device=model.device)
    zeros = lambda k: torch.zeros(k, dtype=torch.float64, device=model.device)
    x = torch.as_tensor(model.meta.x0 if x0 is None else x0, dtype=torch.float64, device=model.device).clone()
    with BarrierLayer(model) as bar, KKTObject(model) as kkt, FilterSearch(bar, **search_opts) as fs, Restoration(fs, **(resto_opts or {})) as resto:
        counts = (bar.info["ncon"], bar.info["nz"])
        counts_r = (bar.info["ncon"], bar.info["nz"] + 2 * bar.info["ncon"])
        state = bar.start(x, model.cons(x))
        y = state[2]
        c, r, f, g = new(m), new(n), new(1), new(n)
        jv, hv = new(int(model.meta.nnzj)), new(int(model.meta.nnzh))
        xt, st, ct, ft, mt, m3, mt3 = new(n), zeros(m), new(m), new(1), new(2), new(3), new(3)
        e0, e_mu = new(8), new(8)
        out = dict(statuses={}, failed=0, rungs_run=0, trials=0, iterations=0, restorations=0, resto_iterations=0, why=None, status=None)
        mu_floor = max(1e-11, tol / 10.0)

        def evaluate():
            model.eval_residual(x, y, 1.0, c=c, out=r, obj=f)
            model.grad(x, g)

        def factor_and_solve(sigma, dcon, rhs, w, dw):
            """the delta_w retry on the inertia, then one refined solve; ``(sol, dw)``"""
            tries = 0
            while True:
                kkt.assemble(hv, jv, sigma, dw, DELTA_C, dcon=dcon, at=(x, y, w))
                _, neg, doubtful = kkt.factor()
                tries += 1
                if (neg == m and doubtful == 0) or tries >= 24:
                    break
                dw = 1e-4 if dw == 0.0 else dw * (100.0 if tries <= 2 else 8.0)
            return kkt.solve(rhs, refine=refine), dw

        def ladder(search, rung):
            sstate = search.state()
            while sstate["status"] == 0:      # ladders of `rungs` rungs, one status word read per ladder
                for _k in range(rungs):
                    rung()
                out["rungs_run"] += rungs
                sstate = search.state()
            return sstate

        def restoration(mu_orig, max_inf):
            """one restoration phase: True when the device said RETURN"""
            mu_r = max(mu_orig, max_inf)
            resto.enter(state, c, mu_r)
            inner = resto.inner
            inner.reset()
            for k in range(resto_max_iter):
                out["resto_iterations"] += 1
                zeta = math.sqrt(mu_r)
                model.eval_residual(x, y, 0.0, c=c, out=r, obj=f)
                changed = False
                while mu_r > 1e-11 and BarrierLayer.optimality_error(resto.error(state, r, c, mu_r, zeta, out=e_mu), counts_r)[0] <= KAPPA_EPS * mu_r:
                    mu_r, changed = max(1e-11, min(KAPPA_MU * mu_r, mu_r ** THETA_MU)), True
                    zeta = math.sqrt(mu_r)
                if changed:
                    inner.reset()
                tau = max(TAU_MIN, 1.0 - mu_r)
                model.jac_hess_coord(x, y, jv, hv, obj_weight=0.0)
                sigma, dcon, rhs = resto.terms(state, r, c, mu_r, zeta)
                sol, _ = factor_and_solve(sigma, dcon, rhs, 0.0, 0.0)
                dirs, alpha = resto.step(state, sol, mu_r, tau, zeta)
                resto.merit(0, state[0], state[1], c, zeta, out=m3)
                resto.begin(state, sol, dirs[0], m3, alpha, mu_r, zeta)

                def rung():
                    resto.trial(state, sol, dirs[0], xt, st)
                    model.cons(xt, ct)
                    resto.merit(1, xt, st, ct, zeta, out=mt3)
                    inner.accept(mt3[0:1], mt3[1:3], mu_r, alpha)
                sstate = ladder(inner, rung)
                if log:
                    log(dict(resto_iter=k, mu=mu_r, status=sstate["status_name"], trials=sstate["trials"], theta_R=sstate["theta0"]))
                if not sstate["status_name"].startswith("accepted"):
                    out["why"] = "inner search failed"
                    return False
                resto.update(state, sol, dirs, alpha, mu_r)
                model.obj_device(x, out=f)
                model.cons(x, c)
                bar.merit(state[0], state[1], c, out=mt)
                resto.check(f, mt, mu_orig)
                if resto.state()["state_name"] == "return":
                    resto.leave(state)
                    out["why"] = "returned"
                    return True
            out["why"] = "no return within the cap"
            return False

        evaluate()
        for it in range(max_iter + 1):
            err = BarrierLayer.optimality_error(bar.error(state, r, c, 0.0, out=e0), counts)
            out.update(iterations=it, error=err[0])
            if log:
                log(dict(iter=it, objective=float(f[0]), error=err[0], dual=err[1], primal=err[2], compl=err[3], mu=mu))
            if err[0] <= tol or it == max_iter:
                out["status"] = "solved" if err[0] <= tol else "max_iter"
                break
            changed = False
            while mu > mu_floor and BarrierLayer.optimality_error(bar.error(state, r, c, mu, out=e_mu), counts)[0] <= KAPPA_EPS * mu:
                mu, changed = max(mu_floor, min(KAPPA_MU * mu, mu ** THETA_MU)), True
            if changed:
                fs.reset()      # a new barrier problem: the filter starts again
            tau = max(TAU_MIN, 1.0 - mu)
            bar.error(state, r, c, mu, out=e_mu)
            model.jac_hess_coord(x, y, jv, hv, obj_weight=1.0)
            sigma, dcon, rhs = bar.terms(state, r, c, mu)
            dw, status = 0.0, None
            for _ in range(8):
                sol, dw = factor_and_solve(sigma, dcon, rhs, 1.0, dw)
                dirs, alpha = bar.step(state, sol, mu, tau)
                fs.begin(state, g, sol, dirs[0], f, e_mu, alpha, mu)

                def rung():
                    fs.trial(state, sol, dirs[0], xt, st)
                    model.obj_device(xt, out=ft)
                    model.cons(xt, ct)
                    bar.merit(xt, st, ct, out=mt)
                    fs.accept(ft, mt, mu, alpha)
                sstate = ladder(fs, rung)
                status = sstate["status_name"]
                out["statuses"][status] = out["statuses"].get(status, 0) + 1
                out["trials"] += sstate["trials"]
                if status.startswith("accepted"):
                    break
                out["failed"] += 1
                dw = 1e-4 if dw == 0.0 else dw * 10.0      # another direction from a more convex model
            if status.startswith("accepted"):
                bar.update(state, sol, dirs, alpha, mu)
                evaluate()
                continue
            if out["restorations"] >= max_restorations:
                out["status"] = "search failed"
                break
            if not restoration(mu, float(e_mu[2])):      # max |inf| of this iterate: read only here
                out["status"] = "restoration failed"
                break
            out["restorations"] += 1
            evaluate()
        out.update(x=x, state=state, objective=float(f[0]), mu=mu)
        return out
