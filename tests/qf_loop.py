"""tests/amu_loop.py with the QUALITY-FUNCTION oracle — TEST INFRASTRUCTURE for tests/test_gpu_qf.py, not part of the package.
`device_rule=True`: BarrierLayer and FilterSearch are bound to a BarrierParameter under an AdaptiveBarrierParameter and a
QualityFunction; per iteration ONE error launch, the two directions (mu = 0 and mu = mu_ref) from ONE two-column back-solve on the
iteration's factors, ONE begin launch, max_section_steps + 4 alpha / value pairs with no decision in between, ONE update launch and
ONE read-back (`state()`).  `device_rule=False`: the twelve words, the state and the two directions are read back,
tests/qf_reference.py's `begin`, `section` and `update` are applied on the host (in the device's summation order, for the device's
grid), and every call is unbound and takes the host's mu and tau.  The two variants must walk through bitwise the same iterates.  The
delta_w retry stays the host's, as in amu_loop.py: the factors the two-column solve uses are those of the first admissible delta_w
of the iteration."""
import contextlib

import numpy as np
import torch

import amu_reference as aref
import barrier_reference as bref
import mu_reference as mref
import qf_reference as qref
from infiniteexamodels.jl_amd.barrier import AdaptiveBarrierParameter, BarrierLayer, BarrierParameter, FilterSearch, QualityFunction
from infiniteexamodels.jl_amd.kkt_chain import KKTObject

DELTA_C = 1e-10


def solve(model, device_rule, x0=None, tol=1e-8, max_iter=200, mu=0.1, rungs=4, refine=1, qf_opts=None, **search_opts):
    """``dict(x, objective, iterations, error, status, statuses, failed, iterates, mu, mus, modes, sigmas, sections, to_fixed, to_free)``;
    `iterates` holds x after every iteration (host copies), `mus` the mu of every iteration, `modes` the mode after every update,
    `sigmas` the section's result and `sections` its (status, evaluations) per iteration"""
    n, m = int(model.meta.nvar), int(model.meta.ncon)
    new = lambda *k: torch.empty(*k, dtype=torch.float64, device=model.device)
    zeros = lambda k: torch.zeros(k, dtype=torch.float64, device=model.device)
    x = torch.as_tensor(model.meta.x0 if x0 is None else x0, dtype=torch.float64, device=model.device).clone()
    host = lambda t: np.array(t.tolist(), dtype=np.float64)
    with BarrierLayer(model) as bar, KKTObject(model) as kkt, FilterSearch(bar, **search_opts) as fs, BarrierParameter(bar, mu_init=mu, tol=tol) as par, \
            AdaptiveBarrierParameter(par) as amu, QualityFunction(amu, **(qf_opts or {})) as qf:
        counts = (bar.info["ncon"], bar.info["nz"])
        n_wg = bar.info["workgroups"]
        opts, aopts = mref.options(mu_init=mu, tol=tol), aref.options()
        qopts = qref.options(aopts, **(qf_opts or {}))
        mu_ref = qopts["mu_ref"]
        blk, ab, qb = mref.fresh_block(opts), aref.fresh_block(aopts), qref.fresh_block()
        B = bref.relaxed_bounds(model.meta.lvar, model.meta.uvar, model.meta.lcon, model.meta.ucon, bar.relax)
        if device_rule:
            bar.bind_mu(par)
            fs.bind_mu(par)
        try:
            state = bar.start(x, model.cons(x))
            y = state[2]
            c, r, f, g = new(m), new(n), new(1), new(n)
            jv, hv = new(int(model.meta.nnzj)), new(int(model.meta.nnzh))
            xt, st, ct, ft, mt = new(n), zeros(m), new(m), new(1), new(2)
            w = new(12)
            sigma, dcon, rhs, rhs2 = new(n), new(m), new(n + m), new(2, n + m)
            dirs0, dirs1, alpha0, alpha1 = tuple(zeros(k) for k in (m, n, n, m, m)), tuple(zeros(k) for k in (m, n, n, m, m)), new(2), new(2)
            out = dict(statuses={}, failed=0, iterations=0, iterates=[], status=None, mus=[], modes=[], sigmas=[], sections=[])

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
                # sigma and dcon do not depend on mu: the factors of this iteration, and the two directions from ONE pass over them
                with amu.affine(bar, fs) if device_rule else contextlib.nullcontext():
                    bar.terms(state, r, c, 0.0, out=(sigma, dcon, rhs2[0]))
                    bar.terms(state, r, c, mu_ref, out=(sigma, dcon, rhs2[1]))
                    dw, tries = factorise(dw, tries)
                    sol2 = kkt.solve(rhs2.t(), refine=refine).t()
                    bar.step(state, sol2[0], 0.0, 1.0, out=dirs0, alpha=alpha0)
                    bar.step(state, sol2[1], mu_ref, 1.0, out=dirs1, alpha=alpha1)
                d0, d1 = (sol2[0], *dirs0), (sol2[1], *dirs1)
                if device_rule:
                    qf.begin(state, r, c, w)
                    qf.section(state, d0, d1)
                    qf.update(w, search=fs)
                    s = qf.state()      # THE read-back
                    mu, tau, status, changed, e0, mode = s["mu"], s["tau"], s["status"], s["changed"], s["e0"], s["mode"]
                    to_fixed, to_free, sig, sec = s["to_fixed"], s["to_free"], s["section"]["sigma"], (s["section"]["status"], s["section"]["evaluations"])
                else:
                    wh, sth = host(w), tuple(host(t) for t in state)
                    h0, h1 = tuple(host(t) for t in d0), tuple(host(t) for t in d1)
                    qb = qref.begin(B, sth, host(r), host(c), wh, ab, aopts, qopts, n_wg)
                    qb = qref.section(B, sth, h0, h1, qb, blk, qopts, n_wg)
                    blk, ab, _ = qref.update(blk, ab, qb, wh, counts, opts, aopts)
                    iw, ia, iq = mref.ints(blk), mref.ints(ab), qref.ints(qb)
                    mu, tau, status, changed, e0, mode = float(blk[0]), float(blk[1]), int(iw[8]), bool(iw[9] & 1), float(blk[3]), int(ia[aref.MODE])
                    to_fixed, to_free, sig, sec = int(ia[aref.TO_FIXED]), int(ia[aref.TO_FREE]), float(qb[qref.BEST]), (int(iq[qref.STATUS]), int(iq[qref.EVALS]))
                    if changed:
                        fs.reset()      # a new barrier problem: the filter starts again
                out.update(iterations=it, error=e0, status=status, mu=mu, to_fixed=to_fixed, to_free=to_free)
                out["mus"].append(mu)
                out["modes"].append(mode)
                out["sigmas"].append(sig)
                out["sections"].append(sec)
                if status != mref.ITERATING or it == max_iter:
                    break
                bar.terms(state, r, c, mu, out=(sigma, dcon, rhs))
                sname, factored = None, True      # (factorised in front of the two-column solve)
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
