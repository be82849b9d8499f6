"""tests/search_loop.py with the barrier parameter as an object — TEST INFRASTRUCTURE for tests/test_gpu_mu.py, not part of the
package.  `device_mu=True`: BarrierLayer and FilterSearch are bound to a BarrierParameter; per iteration ONE error launch, ONE update
launch and ONE read-back (`state()`) give the stopping test, mu and tau, and empty the filter when mu moved.  `device_mu=False`: the
same twelve words are read back, tests/mu_reference.py's `update` is applied on the host, `reset()` is the host's, and every call
is unbound and takes the host's mu and tau.  The two variants must walk through bitwise the same iterates.  The delta_w retry stays
the host's, as in search_loop.py."""
import numpy as np
import torch

import mu_reference as mref
from infiniteexamodels.jl_amd.barrier import BarrierLayer, BarrierParameter, FilterSearch
from infiniteexamodels.jl_amd.kkt_chain import KKTObject

DELTA_C = 1e-10


def solve(model, device_mu, x0=None, tol=1e-8, max_iter=200, mu=0.1, rungs=4, refine=1, **search_opts):
    """``dict(x, objective, iterations, error, status, statuses, failed, iterates, mu, decreases)``; `iterates` holds x after every
    iteration (host copies)"""
    n, m = int(model.meta.nvar), int(model.meta.ncon)
    new = lambda k: torch.empty(k, dtype=torch.float64, device=model.device)
    x = torch.as_tensor(model.meta.x0 if x0 is None else x0, dtype=torch.float64, device=model.device).clone()
    with BarrierLayer(model) as bar, KKTObject(model) as kkt, FilterSearch(bar, **search_opts) as fs, BarrierParameter(bar, mu_init=mu, tol=tol) as par:
        counts = (bar.info["ncon"], bar.info["nz"])
        opts = mref.options(mu_init=mu, tol=tol)
        blk = mref.fresh_block(opts)
        if device_mu:
            bar.bind_mu(par)
            fs.bind_mu(par)
        try:
            state = bar.start(x, model.cons(x))
            y = state[2]
            c, r, f, g = new(m), new(n), new(1), new(n)
            jv, hv = new(int(model.meta.nnzj)), new(int(model.meta.nnzh))
            xt, st, ct, ft, mt = new(n), torch.zeros(m, dtype=torch.float64, device=model.device), new(m), new(1), new(2)
            w = new(12)
            out = dict(statuses={}, failed=0, iterations=0, iterates=[], status=None)

            def evaluate():
                model.eval_residual(x, y, 1.0, c=c, out=r, obj=f)
                model.grad(x, g)

            evaluate()
            for it in range(max_iter + 1):
                par.error(state, r, c, out=w)
                if device_mu:
                    par.update(w, search=fs)
                    s = par.state()      # THE read-back
                    mu, tau, status, changed, e0, decreases = s["mu"], s["tau"], s["status"], s["changed"], s["e0"], s["decreases"]
                else:
                    blk, _ = mref.update(blk, np.array(w.tolist()), counts, opts)      # the read-back, then the restatement on the host
                    iw = mref.ints(blk)
                    mu, tau, status, changed, e0, decreases = float(blk[0]), float(blk[1]), int(iw[8]), bool(iw[9] & 1), float(blk[3]), int(iw[10])
                    if changed:
                        fs.reset()      # a new barrier problem: the filter starts again
                out.update(iterations=it, error=e0, status=status, mu=mu, decreases=decreases)
                if status != mref.ITERATING or it == max_iter:
                    break
                model.jac_hess_coord(x, y, jv, hv, obj_weight=1.0)
                sigma, dcon, rhs = bar.terms(state, r, c, mu)
                dw, tries, sname = 0.0, 0, None
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
                    fs.begin(state, g, sol, dirs[0], f, w[:8], alpha, mu)
                    while True:      # ladders of `rungs` rungs, one status word read per ladder
                        for _k in range(rungs):
                            fs.trial(state, sol, dirs[0], xt, st)
                            model.obj_device(xt, out=ft)
                            model.cons(xt, ct)
                            bar.merit(xt, st, ct, out=mt)
                            fs.accept(ft, mt, mu, alpha)
                        sstate = fs.state()
                        if sstate["status"] != 0:
                            break
                    sname = sstate["status_name"]
                    out["statuses"][sname] = out["statuses"].get(sname, 0) + 1
                    if sname.startswith("accepted"):
                        break
                    out["failed"] += 1
                    dw = 1e-4 if dw == 0.0 else dw * 10.0      # another direction from a more convex model
                if not sname.startswith("accepted"):
                    break
                bar.update(state, sol, dirs, alpha, mu)
                evaluate()
                out["iterates"].append(x.cpu().numpy().copy())
            out.update(x=x, objective=float(f[0]))
            return out
        finally:
            if device_mu:
                fs.bind_mu(None)
                bar.bind_mu(None)
