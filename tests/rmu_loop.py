"""tests/resto_loop.py's interior-point loop with the restoration problem's own barrier parameter — BarrierLayer + kkt_chain.KKTObject
+ FilterSearch + Restoration + RestorationParameter — TEST INFRASTRUCTURE for tests/test_gpu_rmu.py, not part of the package.  Two
ways to decide, over the same device work:

``decide="device"``: the restoration and its inner search are BOUND (``resto.bind_mu(rp)``, ``resto.inner.bind_mu(rp.inner_mu)``);
``rp.enter`` forms mu_R, ``rp.error`` + ``rp.update`` are the rule and the STATIONARY exit, ``rp.trigger`` follows every accept of
both searches, and the host reads ``rp.state()`` and the search's state word.  The scalars it passes to the ``resto.*`` calls are
zeros: nothing looks at them.

``decide="host"``: nothing is bound; the SAME 32 words are read back and tests/rmu_reference.py decides (``update``, ``trigger``,
``enter``); the ``resto.*`` calls get mu, tau and zeta as host doubles, ``inner.reset()`` follows a change of mu.

Both walk through the same iterates bit for bit.  The original problem's mu rule and the delta_w retry stay the host's, as in
tests/resto_loop.py."""
import numpy as np
import torch

import mu_reference as mref
import rmu_reference as qref
import search_reference as sref
from infiniteexamodels.jl_amd.barrier import BarrierLayer, FilterSearch, Restoration, RestorationParameter
from infiniteexamodels.jl_amd.kkt_chain import KKTObject

KAPPA_EPS, KAPPA_MU, THETA_MU, TAU_MIN, DELTA_C = 10.0, 0.2, 1.5, 0.99, 1e-10


def solve(model, x0=None, decide="device", tol=1e-8, max_iter=200, mu=0.1, refine=1, max_restorations=5, resto_max_iter=100, use_trigger=True, log=None):
    """``dict(status, x, objective, iterations, error, restorations, resto_iterations, why, accepts, triggers, decreases, truncated,
    iterates)``; status: "solved" | "max_iter" | "search failed" | "restoration failed" | "locally infeasible" """
    assert decide in ("device", "host")
    on_device = decide == "device"
    n, m = int(model.meta.nvar), int(model.meta.ncon)
    new = lambda k: torch.empty(k, dtype=torch.float64, device=model.device)
    zeros = lambda k: torch.zeros(k, dtype=torch.float64, device=model.device)
    x = torch.as_tensor(model.meta.x0 if x0 is None else x0, dtype=torch.float64, device=model.device).clone()
    with BarrierLayer(model) as bar, KKTObject(model) as kkt, FilterSearch(bar) as fs, Restoration(fs) as resto, RestorationParameter(resto) as rp:
        inner = resto.inner
        if on_device:
            resto.bind_mu(rp)
            inner.bind_mu(rp.inner_mu)
        counts = (bar.info["ncon"], bar.info["nz"])
        counts_r = (bar.info["ncon"], bar.info["nz"] + 2 * bar.info["ncon"])
        state = bar.start(x, model.cons(x))
        y = state[2]
        c, r, f, g = new(m), new(n), new(1), new(n)
        jv, hv = new(int(model.meta.nnzj)), new(int(model.meta.nnzh))
        xt, st, ct, ft, mt, m3, mt3 = new(n), zeros(m), new(m), new(1), new(2), new(3), new(3)
        e0, e_mu, w32 = new(8), new(8), new(32)
        out = dict(iterations=0, restorations=0, resto_iterations=0, why=None, status=None, accepts=0, decreases=[], truncated=False, iterates=[], e0=[])
        trig = [0, 0]
        own = qref.fresh_own()      # the host's copy of the own block (decide="host")
        mu_floor = max(1e-11, tol / 10.0)

        def evaluate():
            model.eval_residual(x, y, 1.0, c=c, out=r, obj=f)
            model.grad(x, g)

        def factor_and_solve(sigma, dcon, rhs, w, dw):
            tries = 0
            while True:
                kkt.assemble(hv, jv, sigma, dw, DELTA_C, dcon=dcon, at=(x, y, w))
                _, neg, doubtful = kkt.factor()
                tries += 1
                if (neg == m and doubtful == 0) or tries >= 24:
                    break
                dw = 1e-4 if dw == 0.0 else dw * (100.0 if tries <= 2 else 8.0)
            return kkt.solve(rhs, refine=refine), dw

        def ladder(search, which, rung, alpha):
            """rungs of one accept each, the trigger behind every accept, one state read per rung; the state the search ends in"""
            nonlocal own
            sstate = search.state()
            while sstate["status"] == 0:
                rung()
                out["accepts"] += 1
                if on_device:
                    if use_trigger:
                        rp.trigger(which, alpha)
                    sstate = search.state()
                else:
                    sstate = search.state()
                    if use_trigger and sstate["status"] == 0:
                        ctl = sref.block(alpha=sstate["alpha"], theta0=sstate["theta0"], slope=sstate["slope"], theta_min=sstate["theta_min"], status=sref.SEARCHING)
                        own, ctl, a0 = qref.trigger(own, ctl, which)
                        if a0 is not None:      # fired: what the device would have written into the block
                            sstate = dict(sstate, status=sref.FAILED, status_name="failed", alpha=0.0)
                            trig[which] += 1
            return sstate

        def restoration(mu_orig, err8):
            """one restoration phase: True when the device said RETURN"""
            nonlocal own
            if on_device:
                rp.enter(err8, mu_orig)
                resto.enter(state, c, 0.0)
                first = rp.state()
                if first["status_name"] == "unusable":
                    out["why"] = "unusable"
                    return False
                mu_r = tau = zeta = 0.0
            else:
                own, mblk, _ = qref.enter(own, mref.fresh_block(dict(qref.OPTS, mu_init=0.1)), sref.block(), err8.cpu().numpy(), mu_orig)
                if qref.ints(own)[qref.STATUS] == qref.UNUSABLE:
                    out["why"] = "unusable"
                    return False
                mu_r, tau, zeta = (float(v) for v in mblk[:3])
                rp.inner_mu.reset(mu_r)      # (only iem_rmu_error reads it here: the candidates start from this block)
                resto.enter(state, c, mu_r)
                inner.reset()
            for k in range(resto_max_iter):
                out["resto_iterations"] += 1
                out["iterates"].append(x.cpu().numpy().copy())
                model.eval_residual(x, y, 0.0, c=c, out=r, obj=f)
                rp.error(state, r, c, out=w32)
                if on_device:
                    rp.update(w32)
                    s = rp.state()
                    status, last, truncated, e_0 = s["status"], s["decreases_last"], s["truncated"], s["e0"]
                else:
                    own, mblk, _ = qref.update(own, mblk, sref.block(), w32.cpu().numpy(), counts_r)
                    status, last, truncated, e_0 = int(qref.ints(own)[qref.STATUS]), int(qref.ints(own)[qref.LAST]), bool(qref.ints(own)[qref.FLAGS] & 2), float(own[qref.E0])
                    if last:
                        mu_r, tau, zeta = (float(v) for v in mblk[:3])
                        rp.inner_mu.reset(mu_r)
                        inner.reset()
                out["decreases"].append(int(last))
                out["truncated"] = out["truncated"] or bool(truncated)
                out["e0"].append(float(e_0))
                if status != qref.ITERATING:
                    out["why"] = "stationary" if status == qref.STATIONARY else "unusable"
                    return False
                model.jac_hess_coord(x, y, jv, hv, obj_weight=0.0)
                sigma, dcon, rhs = resto.terms(state, r, c, mu_r, zeta)
                sol, _ = factor_and_solve(sigma, dcon, rhs, 0.0, 0.0)
                dirs, alpha = resto.step(state, sol, mu_r, tau if tau else 1.0, zeta)
                resto.merit(0, state[0], state[1], c, zeta, out=m3)
                resto.begin(state, sol, dirs[0], m3, alpha, mu_r, zeta)

                def rung():
                    resto.trial(state, sol, dirs[0], xt, st)
                    model.cons(xt, ct)
                    resto.merit(1, xt, st, ct, zeta, out=mt3)
                    inner.accept(mt3[0:1], mt3[1:3], mu_r, alpha)
                sstate = ladder(inner, 1, rung, alpha)
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
                if (rp.state()["resto_state_name"] if on_device else resto.state()["state_name"]) == "return":
                    resto.leave(state)
                    out["why"] = "returned"
                    return True
            out["why"] = "no return within the cap"
            return False

        evaluate()
        for it in range(max_iter + 1):
            err = BarrierLayer.optimality_error(bar.error(state, r, c, 0.0, out=e0), counts)
            out.update(iterations=it, error=err[0])
            out["iterates"].append(x.cpu().numpy().copy())
            if log:
                log(dict(iter=it, objective=float(f[0]), error=err[0], mu=mu))
            if err[0] <= tol or it == max_iter:
                out["status"] = "solved" if err[0] <= tol else "max_iter"
                break
            changed = False
            while mu > mu_floor and BarrierLayer.optimality_error(bar.error(state, r, c, mu, out=e_mu), counts)[0] <= KAPPA_EPS * mu:
                mu, changed = max(mu_floor, min(KAPPA_MU * mu, mu ** THETA_MU)), True
            if changed:
                fs.reset()
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
                status = ladder(fs, 0, rung, alpha)["status_name"]
                if status.startswith("accepted"):
                    break
                dw = 1e-4 if dw == 0.0 else dw * 10.0
            if status.startswith("accepted"):
                bar.update(state, sol, dirs, alpha, mu)
                evaluate()
                continue
            if out["restorations"] >= max_restorations:
                out["status"] = "search failed"
                break
            if on_device:      # (enter zeroes the own block: the triggers of the original search counted so far are carried over)
                s = rp.state()
                trig[0] += s["triggers_orig"]
                trig[1] += s["triggers_inner"]
            if not restoration(mu, e_mu):
                out["status"] = "locally infeasible" if out["why"] == "stationary" else "restoration failed"
                break
            out["restorations"] += 1
            evaluate()
        if on_device:
            s = rp.state()
            trig[0] += s["triggers_orig"]
            trig[1] += s["triggers_inner"]
            inner.bind_mu(None)
            resto.bind_mu(None)
        out.update(x=x.cpu().numpy().copy(), objective=float(f[0]), mu=mu, triggers=tuple(trig))
        return out
