"""tests/amu_loop.py (probing oracle) with MEHROTRA'S CORRECTOR — TEST INFRASTRUCTURE for tests/test_gpu_mpc.py, not part of the
package.  Behind the rule's update: ONE mpc_terms launch (two columns), ONE two-column refined solve on the iteration's factors,
barrier_step on column 0, mpc_step on column 1, ONE probe of the corrected direction and ONE mpc_select launch; the search, the
rungs and the update run on the first-order buffers as before.  `device_rule=True`: the objects are bound, the rule and the
decision run on the device and the host reads `amu.state()` (and `mpc.state()` for the counts).  `device_rule=False`: the words are
read back, tests/amu_reference.py's `update` and tests/mpc_reference.py's `decide` are applied on the host, the copy is the host's,
and every call is unbound and takes the host's mu and tau.  The two variants must walk through bitwise the same iterates.
`corrector=False` is amu_loop.py's sequence (for the iteration counts beside it).  A failed search retries with a larger delta_w on
the same two columns: the affine direction stays that of the iteration's first factors."""
import contextlib

import numpy as np
import torch

import amu_reference as aref
import mpc_reference as pref
import mu_reference as mref
from infiniteexamodels.jl_amd.barrier import AdaptiveBarrierParameter, BarrierLayer, BarrierParameter, FilterSearch, MehrotraCorrector
from infiniteexamodels.jl_amd.kkt_chain import KKTObject

DELTA_C = 1e-10


def solve(model, device_rule, corrector=True, x0=None, tol=1e-8, max_iter=200, mu=0.1, rungs=4, refine=1, bounds=None, **search_opts):
    """``dict(x, objective, iterations, error, status, statuses, failed, iterates, mu, mus, taken, refused, decisions)``; `iterates`
    holds x after every iteration (host copies), `decisions` the decision of every select"""
    n, m = int(model.meta.nvar), int(model.meta.ncon)
    new = lambda k: torch.empty(k, dtype=torch.float64, device=model.device)
    zeros = lambda k: torch.zeros(k, dtype=torch.float64, device=model.device)
    x = torch.as_tensor(model.meta.x0 if x0 is None else x0, dtype=torch.float64, device=model.device).clone()
    with BarrierLayer(model, bounds=bounds) as bar, KKTObject(model) as kkt, FilterSearch(bar, **search_opts) as fs, BarrierParameter(bar, mu_init=mu, tol=tol) as par, \
            AdaptiveBarrierParameter(par) as amu, MehrotraCorrector(amu) as mpc:
        counts = (bar.info["ncon"], bar.info["nz"])
        opts, aopts, mopts = mref.options(mu_init=mu, tol=tol), aref.options(), pref.options()
        blk, ab = mref.fresh_block(opts), aref.fresh_block(aopts)
        lcon, ucon = (np.asarray(a, dtype=np.float64) for a in ((bounds[2], bounds[3]) if bounds is not None else (model.meta.lcon, model.meta.ucon)))
        ine = torch.as_tensor(lcon != ucon, device=model.device)      # the inequality rows: what the host's copy of the slack side takes
        if device_rule:
            bar.bind_mu(par)
            fs.bind_mu(par)
            mpc.bind_mu(par)
        try:
            state = bar.start(x, model.cons(x))
            y = state[2]
            c, r, f, g = new(m), new(n), new(1), new(n)
            jv, hv = new(int(model.meta.nnzj)), new(int(model.meta.nnzh))
            xt, st, ct, ft, mt = new(n), zeros(m), new(m), new(1), new(2)
            w, q, q_c = new(12), new(4), new(4)
            sigma, dcon, rhs_a, rhs2 = new(n), new(m), new(n + m), torch.empty((2, n + m), dtype=torch.float64, device=model.device)
            dirs_a, alpha_a = tuple(zeros(k) for k in (m, n, n, m, m)), new(2)
            dirs, alpha = tuple(zeros(k) for k in (m, n, n, m, m)), new(2)
            dirs_c, alpha_c = tuple(zeros(k) for k in (m, n, n, m, m)), new(2)
            out = dict(statuses={}, failed=0, iterations=0, iterates=[], status=None, mus=[], taken=0, refused=0, decisions=[])

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
                with amu.affine(bar, fs) if device_rule else contextlib.nullcontext():
                    bar.terms(state, r, c, 0.0, out=(sigma, dcon, rhs_a))
                    dw, tries = factorise(dw, tries)
                    sol_a = kkt.solve(rhs_a, refine=refine)
                    bar.step(state, sol_a, 0.0, 1.0, out=dirs_a, alpha=alpha_a)
                    amu.probe(state, sol_a, dirs_a, alpha_a, out=q)
                if device_rule:
                    amu.update(w, q, search=fs)
                    s = amu.state()      # THE read-back
                    mu, tau, status, changed, e0 = s["mu"], s["tau"], s["status"], s["changed"], s["e0"]
                else:
                    blk, ab, _ = aref.update(blk, ab, np.array(w.tolist()), np.array(q.tolist()), counts, opts, aopts)
                    iw = mref.ints(blk)
                    mu, tau, status, changed, e0 = float(blk[0]), float(blk[1]), int(iw[8]), bool(iw[9] & 1), float(blk[3])
                    if changed:
                        fs.reset()      # a new barrier problem: the filter starts again
                out.update(iterations=it, error=e0, status=status, mu=mu)
                out["mus"].append(mu)
                if status != mref.ITERATING or it == max_iter:
                    break
                mpc.terms(state, r, c, sol_a, dirs_a, mu, out=rhs2)
                sname, factored = None, True
                for _ in range(8):
                    if not factored:
                        dw, tries = factorise(dw, tries)
                    factored = False
                    sol2 = kkt.solve(rhs2.t(), refine=refine).t()      # (2, n + m), rows contiguous: ONE pass for both columns
                    sol = sol2[0]
                    bar.step(state, sol, mu, tau, out=dirs, alpha=alpha)
                    if corrector:
                        mpc.step(state, sol_a, dirs_a, sol2[1], mu, tau, out=dirs_c, alpha=alpha_c)
                        amu.probe(state, sol2[1], dirs_c, alpha_c, out=q_c)
                        if device_rule:
                            mpc.select(q_c, alpha_c, sol2[1], dirs_c, sol, dirs, alpha)
                            t = mpc.state()
                            taken = t["taken"]
                        else:
                            taken = bool(pref.decide(np.array(q_c.tolist()), np.array(alpha_c.tolist()), ab[aref.AVG], counts[1], mopts)[0])
                            if taken:
                                sol.copy_(sol2[1])
                                dirs[1].copy_(dirs_c[1]); dirs[2].copy_(dirs_c[2])
                                for k in (0, 3, 4):
                                    dirs[k][ine] = dirs_c[k][ine]
                                alpha.copy_(alpha_c)
                        out["decisions"].append(taken)
                        out["taken" if taken else "refused"] += 1
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
            if device_rule and corrector:
                t = mpc.state()
                assert (t["n_taken"], t["n_refused"]) == (out["taken"], out["refused"])      # the device's counters are the host's tally
            out.update(x=x, objective=float(f[0]))
            return out
        finally:
            if device_rule:
                mpc.bind_mu(None)
                fs.bind_mu(None)
                bar.bind_mu(None)
