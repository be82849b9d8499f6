"""tests/mu_loop.py's sequence (the barrier parameter on the device, everything bound) with the starting point as an object — TEST
INFRASTRUCTURE for tests/test_gpu_init.py, not part of the package.

`start=None`: iem_barrier_start alone, y = 0 — mu_loop.solve(device_mu=True).
`start="ls"`: behind iem_barrier_start the least-squares estimate — iem_init_ls_terms, assemble with a ZERO Hessian value array, factor,
    one refined solve, iem_init_ls_apply; then the residual again, because y moved.
`start="warm"`: in the place of iem_barrier_start the projection of `warm_state` (host arrays x, s, y, zL, zU, vL, vU) —
    iem_init_warm, the evaluation, iem_mu_error, iem_init_mu: the loop begins at the mu0 the device chose.
The delta_w retry stays the host's, as in mu_loop.py."""
import numpy as np
import torch

import mu_reference as mref
from infiniteexamodels.jl_amd.barrier import BarrierLayer, BarrierParameter, FilterSearch, StartingPoint
from infiniteexamodels.jl_amd.kkt_chain import KKTObject

DELTA_C = 1e-10


def solve(model, start=None, warm_state=None, bounds=None, x0=None, tol=1e-8, max_iter=200, mu=0.1, rungs=4, refine=1, init_opts=None, **search_opts):
    """``dict(x, objective, iterations, error, status, statuses, failed, mu, decreases, final, init, mus)``; `final` is the state at
    the end on the host, `init` what the starting point did: for "ls" ``ynorm_host`` (the host's max |y + delta|), ``y_start`` and the
    object's state; for "warm" the twelve words ``w`` at the warm state, ``mu_start`` (word 0 of the parameter's block behind
    iem_init_mu) and the object's state"""
    n, m = int(model.meta.nvar), int(model.meta.ncon)
    new = lambda k: torch.empty(k, dtype=torch.float64, device=model.device)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=model.device).clone()
    with BarrierLayer(model, bounds=bounds) as bar, KKTObject(model) as kkt, FilterSearch(bar, **search_opts) as fs, BarrierParameter(bar, mu_init=mu, tol=tol) as par, \
            StartingPoint(bar, **(init_opts or {})) as init:
        bar.bind_mu(par)
        fs.bind_mu(par)
        try:
            c, r, f, g = new(m), new(n), new(1), new(n)
            jv, hv = new(int(model.meta.nnzj)), new(int(model.meta.nnzh))
            xt, st, ct, ft, mt = new(n), torch.zeros(m, dtype=torch.float64, device=model.device), new(m), new(1), new(2)
            w = new(12)
            out = dict(statuses={}, failed=0, iterations=0, status=None, mus=[], init={})
            if start == "warm":
                state = tuple(dev(a) for a in warm_state)
                init.warm(state)
            else:
                x = dev(model.meta.x0 if x0 is None else x0)
                state = bar.start(x, model.cons(x))
            x, y = state[0], state[2]

            def evaluate():
                model.eval_residual(x, y, 1.0, c=c, out=r, obj=f)
                model.grad(x, g)

            evaluate()
            if start == "ls":
                zeros_h, zeros_y = torch.zeros_like(hv), torch.zeros_like(y)
                model.jac_hess_coord(x, y, jv, hv, obj_weight=1.0)
                sigma, dcon, rhs = init.ls_terms(state, r)
                kkt.assemble(zeros_h, jv, sigma, 0.0, DELTA_C, dcon=dcon, at=(x, zeros_y, 0.0))      # W = 0 at (y = 0, obj_weight = 0): the refinement stays matrix-free
                inertia = kkt.factor()
                sol = kkt.solve(rhs, refine=refine)
                ynorm_host = float((y + sol[n:]).abs().max()) if m else 0.0
                init.ls_apply(sol, y)
                out["init"] = dict(init.state(), ynorm_host=ynorm_host, inertia=inertia, y_start=y.cpu().numpy().copy())
                evaluate()
            elif start == "warm":
                par.error(state, r, c, out=w)
                init.mu(w, par)
                out["init"] = dict(init.state(), w=np.array(w.tolist()), mu_start=par.state()["mu"], state=tuple(t.cpu().numpy().copy() for t in state))
            for it in range(max_iter + 1):
                par.error(state, r, c, out=w)
                par.update(w, search=fs)
                s = par.state()      # THE read-back
                mu, tau, status, e0, decreases = s["mu"], s["tau"], s["status"], s["e0"], s["decreases"]
                out.update(iterations=it, error=e0, status=status, mu=mu, decreases=decreases)
                out["mus"].append(mu)
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
            out.update(x=x, objective=float(f[0]), final=tuple(t.cpu().numpy().copy() for t in state))
            return out
        finally:
            fs.bind_mu(None)
            bar.bind_mu(None)
