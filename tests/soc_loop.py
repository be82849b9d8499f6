"""tests/search_loop.py's interior-point loop with the second-order correction — BarrierLayer + kkt_chain.KKTObject + FilterSearch +
SecondOrderCorrection — TEST INFRASTRUCTURE for tests/test_gpu_soc.py, not part of the package.  The host keeps what search_loop.py
keeps (the monotone mu rule, the delta_w retry, reset() whenever mu changes) and reads back what it reads, plus ONE word per
correction: behind the first rung it reads the block, and runs rounds of the correction while the device says ACTIVE.  `max_soc = 0`
leaves every SOC call out: the loop of search_loop.py with a first ladder of one rung.  No restoration phase, no scaling."""
import torch

from infiniteexamodels.jl_amd.barrier import BarrierLayer, FilterSearch, SecondOrderCorrection
from infiniteexamodels.jl_amd.kkt_chain import KKTObject

KAPPA_EPS, KAPPA_MU, THETA_MU, TAU_MIN, DELTA_C = 10.0, 0.2, 1.5, 0.99, 1e-10


def solve(model, x0=None, y0=None, tol=1e-8, max_iter=200, mu=0.1, rungs=4, refine=1, max_soc=4, kappa_soc=0.99, log=None, **search_opts):
    """``dict(x, state, objective, iterations, error, statuses, failed, rungs_run, trials, soc_opened, soc_accepted, soc_rounds)``;
    `trials` counts the rejected trials of the backtracking search, `soc_accepted` the searches a corrected step ended"""
    n, m = int(model.meta.nvar), int(model.meta.ncon)
    new = lambda k: torch.empty(k, dtype=torch.float64, device=model.device)
    x = torch.as_tensor(model.meta.x0 if x0 is None else x0, dtype=torch.float64, device=model.device).clone()
    with BarrierLayer(model) as bar, KKTObject(model) as kkt, FilterSearch(bar, **search_opts) as fs:
        soc = SecondOrderCorrection(fs, max_soc=max_soc, kappa_soc=kappa_soc) if max_soc > 0 else None
        counts = (bar.info["ncon"], bar.info["nz"])
        state = bar.start(x, model.cons(x))
        y = state[2]
        if y0 is not None:
            y.copy_(torch.as_tensor(y0, dtype=torch.float64, device=model.device))
        c, r, f, g = new(m), new(n), new(1), new(n)
        jv, hv = new(int(model.meta.nnzj)), new(int(model.meta.nnzh))
        xt, st, ct, ft, mt = new(n), torch.zeros(m, dtype=torch.float64, device=model.device), new(m), new(1), new(2)
        rhs_soc, sol_soc, alpha_soc = new(n + m), new(n + m), new(2)
        dirs_soc = (torch.zeros(m, dtype=torch.float64, device=model.device), new(n), new(n), torch.zeros(m, dtype=torch.float64, device=model.device),
                    torch.zeros(m, dtype=torch.float64, device=model.device))
        e0, e_mu = new(8), new(8)
        out = dict(statuses={}, failed=0, rungs_run=0, trials=0, iterations=0, soc_opened=0, soc_accepted=0, soc_rounds=0)
        mu_floor = max(1e-11, tol / 10.0)

        def evaluate():
            model.eval_residual(x, y, 1.0, c=c, out=r, obj=f)
            model.grad(x, g)

        def rung():
            fs.trial(state, sol, dirs[0], xt, st)
            model.obj_device(xt, out=ft)
            model.cons(xt, ct)
            bar.merit(xt, st, ct, out=mt)
            fs.accept(ft, mt, mu, alpha)

        evaluate()
        try:
            for it in range(max_iter + 1):
                err = BarrierLayer.optimality_error(bar.error(state, r, c, 0.0, out=e0), counts)
                out.update(iterations=it, error=err[0])
                if log:
                    log(dict(iter=it, objective=float(f[0]), error=err[0], dual=err[1], primal=err[2], compl=err[3], mu=mu))
                if err[0] <= tol or it == max_iter:
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
                dw, tries, status = 0.0, 0, None
                for _ in range(8):
                    while True:
                        kkt.assemble(hv, jv, sigma, dw, DELTA_C, dcon=dcon, at=(x, y, 1.0))
                        _, neg, doubtful = kkt.factor()
                        tries += 1
                        if (neg == m and doubtful == 0) or tries >= 24:
                            break
                        dw = 1e-4 if dw == 0.0 else dw * (100.0 if tries <= 2 else 8.0)
                    sol = kkt.solve(rhs, refine=refine)
                    dirs, alpha = bar.step(state, sol, mu, tau)
                    fs.begin(state, g, sol, dirs[0], f, e_mu, alpha, mu)
                    rung()      # the first rung alone, then the correction where the device opens it
                    out["rungs_run"] += 1
                    if soc is not None:
                        soc.open()
                        q = soc.state()
                        out["soc_opened"] += q["state_name"] == "active"
                        while q["state_name"] == "active":
                            soc.rhs(state, c, ct, st, rhs, mu, out=rhs_soc)
                            sol_soc.copy_(kkt.solve(rhs_soc, refine=refine))
                            bar.step(state, sol_soc, mu, tau, out=dirs_soc, alpha=alpha_soc)
                            soc.trial(state, sol_soc, dirs_soc[0], alpha_soc, xt, st)
                            model.obj_device(xt, out=ft)
                            model.cons(xt, ct)
                            bar.merit(xt, st, ct, out=mt)
                            soc.accept(ft, mt, alpha_soc, mu, alpha)
                            out["soc_rounds"] += 1
                            q = soc.state()
                        out["soc_accepted"] += q["state_name"] == "accepted"
                        soc.select(sol_soc, dirs_soc, sol, dirs)
                    sstate = fs.state()
                    while sstate["status"] == 0:      # ladders of `rungs` rungs, one status word read per ladder
                        for _k in range(rungs):
                            rung()
                        out["rungs_run"] += rungs
                        sstate = fs.state()
                    status = sstate["status_name"]
                    out["statuses"][status] = out["statuses"].get(status, 0) + 1
                    out["trials"] += sstate["trials"]
                    if status.startswith("accepted"):
                        break
                    out["failed"] += 1
                    dw = 1e-4 if dw == 0.0 else dw * 10.0      # another direction from a more convex model
                if not status.startswith("accepted"):
                    break
                bar.update(state, sol, dirs, alpha, mu)
                evaluate()
        finally:
            if soc is not None:
                soc.close()
        out.update(x=x, state=state, objective=float(f[0]), mu=mu)
        return out
