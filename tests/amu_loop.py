"""tests/mu_loop.py with the ADAPTIVE barrier parameter — TEST INFRASTRUCTURE for tests/test_gpu_amu.py, not part of the package.
`device_rule=True`: BarrierLayer and FilterSearch are bound to a BarrierParameter that an AdaptiveBarrierParameter drives; per
iteration ONE error launch, (probing oracle) the affine-scaling direction from one more back-solve on the iteration's factors and ONE
probe launch, ONE update launch and ONE read-back (`state()`).  `device_rule=False`: the twelve and the four words are read back,
tests/amu_reference.py's `update` is applied on the host, `reset()` is the host's, and every call is unbound and takes the host's mu
and tau.  The two variants must walk through bitwise the same iterates.  The delta_w retry stays the host's, as in mu_loop.py: the
factors the affine solve uses are those of the first admissible delta_w of the iteration."""
import contextlib

import numpy as np
import torch

import amu_reference as aref
import mu_reference as mref
from infiniteexamodels.jl_amd.barrier import AdaptiveBarrierParameter, BarrierLayer, BarrierParameter, FilterSearch
from infiniteexamodels.jl_amd.kkt_chain import KKTObject

DELTA_C = 1e-10


def solve(model, device_rule, oracle, x0=None, tol=1e-8, max_iter=200, mu=0.1, rungs=4, refine=1, **search_opts):
    """``dict(x, objective, iterations, error, status, statuses, failed, iterates, mu, mus, modes, to_fixed, to_free)``; `iterates` holds
    x after every iteration (host copies), `mus` the mu of every iteration, `modes` the mode after every update"""
    n, m = int(model.meta.nvar), int(model.meta.ncon)
    new = lambda k: torch.empty(k, dtype=torch.float64, device=model.device)
    x = torch.as_tensor(model.meta.x0 if x0 is None else x0, dtype=torch.float64, device=model.device).clone()
    probing = oracle == aref.PROBING
    with BarrierLayer(model) as bar, KKTObject(model) as kkt, FilterSearch(bar, **search_opts) as fs, BarrierParameter(bar, mu_init=mu, tol=tol) as par, \
            AdaptiveBarrierParameter(par, oracle=oracle) as amu:
        counts = (bar.info["ncon"], bar.info["nz"])
        opts, aopts = mref.options(mu_init=mu, tol=tol), aref.options(oracle=oracle)
        blk, ab = mref.fresh_block(opts), aref.fresh_block(aopts)
        if device_rule:
            bar.bind_mu(par)
            fs.bind_mu(par)
        try:
            state = bar.start(x, model.cons(x))
            y = state[2]
            c, r, f, g = new(m), new(n), new(1), new(n)
            jv, hv = new(int(model.meta.nnzj)), new(int(model.meta.nnzh))
            xt, st, ct, ft, mt = new(n), torch.zeros(m, dtype=torch.float64, device=model.device), new(m), new(1), new(2)
            w, q = new(12), new(4)
            sigma, dcon, rhs, rhs_a = new(n), new(m), new(n + m), new(n + m)
            dirs_a, alpha_a = tuple(torch.zeros(k, dtype=torch.float64, device=model.device) for k in (m, n, n, m, m)), new(2)
            out = dict(statuses={}, failed=0, iterations=0, iterates=[], status=None, mus=[], modes=[])

            def evaluate():
                model.eval_residual(x, y, 1.0, c=c, out=r, obj=f)
                model.grad(x, g)

            def factorise(dw, tries):
                while True:
                    kkt.assemble(hv, jv, sigma, dw, DELTA_C, dcon=dcon, at=(x, y, 1.0))
                    _, neg, doubtful = kkt.factor()
                    tries += 1
                    if (neg == m and doubtful == 0) or tries >= 24:
                        return dw, tries
                    dw = 1e-4 if dw == 0.0 else dw * (100.0 if tries <= 2 else 8.0)

            evaluate()
            for it in range(max_iter + 1):
                par.error(state, r, c, out=w)
                model.jac_hess_coord(x, y, jv, hv, obj_weight=1.0)
                dw, tries = 0.0, 0
                if probing:
                    # sigma and dcon do not depend on mu: the factors of this iteration, and the affine-scaling direction from them
                    with amu.affine(bar, fs) if device_rule else contextlib.nullcontext():
                        bar.terms(state, r, c, 0.0, out=(sigma, dcon, rhs_a))
                        dw, tries = factorise(dw, tries)
                        sol_a = kkt.solve(rhs_a, refine=refine)
                        bar.step(state, sol_a, 0.0, 1.0, out=dirs_a, alpha=alpha_a)
                        amu.probe(state, sol_a, dirs_a, alpha_a, out=q)
                if device_rule:
                    amu.update(w, q if probing else None, search=fs)
                    s = amu.state()      # THE read-back
                    mu, tau, status, changed, e0, mode = s["mu"], s["tau"], s["status"], s["changed"], s["e0"], s["mode"]
                    to_fixed, to_free = s["to_fixed"], s["to_free"]
                else:
                    blk, ab, _ = aref.update(blk, ab, np.array(w.tolist()), np.array(q.tolist()) if probing else None, counts, opts, aopts)
                    iw, ia = mref.ints(blk), mref.ints(ab)
                    mu, tau, status, changed, e0, mode = float(blk[0]), float(blk[1]), int(iw[8]), bool(iw[9] & 1), float(blk[3]), int(ia[aref.MODE])
                    to_fixed, to_free = int(ia[aref.TO_FIXED]), int(ia[aref.TO_FREE])
                    if changed:
                        fs.reset()      # a new barrier problem: the filter starts again
                out.update(iterations=it, error=e0, status=status, mu=mu, to_fixed=to_fixed, to_free=to_free)
                out["mus"].append(mu)
                out["modes"].append(mode)
                if status != mref.ITERATING or it == max_iter:
                    break
                bar.terms(state, r, c, mu, out=(sigma, dcon, rhs))
                sname, factored = None, probing      # (the probing variant factorised in front of the affine solve)
                for _ in range(8):
                    if not factored:
                        dw, tries = factorise(dw, tries)
                    factored = False
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
            if device_rule:
                fs.bind_mu(None)
                bar.bind_mu(None)

