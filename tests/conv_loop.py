"""tests/init_loop.py's sequence (the barrier parameter on the device, everything bound, iem_barrier_start) with the stopping test as an
object — TEST INFRASTRUCTURE for tests/test_gpu_conv.py, not part of the package.

Per iteration: iem_mu_error, iem_conv_check, iem_conv_keep, iem_mu_update, and `conv.state()` as THE read-back; behind the solve of the
direction iem_conv_step.  The loop stops on the status word of the iem_conv block and on nothing else (iem_mu_update's own CONVERGED is
not looked at; `limit` only bounds a broken run).  Beside the device THE REFERENCE decides on the host: the same twelve words, f, x (and
x, s, sol, ds, mu behind the step) are read back and tests/conv_reference.py is applied to its own block — device and host must go
through identical decisions, block for block.  Whenever the reference asks for a copy, the host copies the state: `ref_kept`.

`past_latch`: that many further iterations behind a terminal status (the kernels of the loop are not frozen by the latch), each
followed by check, keep and step — the blocks and the kept buffers must not move.  The delta_w retry stays the host's, as in
mu_loop.py."""
import numpy as np
import torch

import conv_reference as cref
import mu_reference as mref
from infiniteexamodels.jl_amd.barrier import BarrierLayer, BarrierParameter, ConvergenceCheck, FilterSearch
from infiniteexamodels.jl_amd.kkt_chain import KKTObject

DELTA_C = 1e-10


def solve(model, tol=1e-8, mu=0.1, rungs=4, refine=1, limit=200, past_latch=0, **conv_opts):
    """``dict(status, checks, iterations, state (the device's conv.state()), block, ref_block, blocks_agree, kept (host copies of the
    object's buffers), ref_kept, ref_kept_at, final (the state at the stop, host), restored (restore into NaN-poisoned vectors, host),
    B, moved_past_latch)``"""
    n, m = int(model.meta.nvar), int(model.meta.ncon)
    new = lambda k: torch.empty(k, dtype=torch.float64, device=model.device)
    host = lambda ts: tuple(t.cpu().numpy().copy() for t in ts)
    x = torch.as_tensor(model.meta.x0, dtype=torch.float64, device=model.device).clone()
    with BarrierLayer(model) as bar, KKTObject(model) as kkt, FilterSearch(bar) as fs, BarrierParameter(bar, mu_init=mu, tol=tol) as par, \
            ConvergenceCheck(par, **conv_opts) as conv:
        import barrier_reference as bref
        import test_gpu_mu as tm
        B = bref.relaxed_bounds(*(np.array(getattr(model.meta, k), dtype=np.float64) for k in ("lvar", "uvar", "lcon", "ucon")), bar.relax)
        counts = (bar.info["ncon"], bar.info["nz"])
        mo, co = mref.options(mu_init=mu, tol=tol), cref.options(**conv_opts)
        ref = cref.fresh_block()
        bar.bind_mu(par)
        fs.bind_mu(par)
        try:
            state = bar.start(x, model.cons(x))
            y = state[2]
            c, r, f, g = new(m), new(n), new(1), new(n)
            jv, hv = new(int(model.meta.nnzj)), new(int(model.meta.nnzh))
            xt, st, ct, ft, mt = new(n), torch.zeros(m, dtype=torch.float64, device=model.device), new(m), new(1), new(2)
            w = new(12)
            out = dict(B=B, blocks_agree=True, ref_kept=None, ref_kept_at=None, iterations=0, moved_past_latch=[])
            block = lambda: tm.peek(conv.device(), cref.WORDS)

            def evaluate():
                model.eval_residual(x, y, 1.0, c=c, out=r, obj=f)
                model.grad(x, g)

            def check():
                nonlocal ref
                par.error(state, r, c, out=w)
                conv.check(w, f, x)
                conv.keep(state)
                par.update(w, search=fs)
                s = conv.state()      # THE read-back
                ref = cref.check(ref, np.array(w.tolist()), float(f[0]), x.cpu().numpy(), counts, co, mo)
                if cref.ints(ref)[cref.KEEP]:
                    out["ref_kept"], out["ref_kept_at"] = host(state), int(cref.ints(ref)[cref.KEPT_AT])
                out["blocks_agree"] &= tm.same_bits(block(), ref)
                return s

            def direction():
                """one iteration behind the check: the direction, iem_conv_step, the search, the update, the evaluation; False where no
                step was accepted"""
                nonlocal ref
                ps = par.state()      # (bound: the calls below ignore these two; the reference's step needs mu)
                mu_now, tau_now = ps["mu"], ps["tau"]
                model.jac_hess_coord(x, y, jv, hv, obj_weight=1.0)
                sigma, dcon, rhs = bar.terms(state, r, c, mu_now)
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
                    dirs, alpha = bar.step(state, sol, mu_now, tau_now)
                    conv.step(state, sol, dirs[0])
                    ref = cref.step(ref, B, x.cpu().numpy(), state[1].cpu().numpy(), sol.cpu().numpy(), dirs[0].cpu().numpy(), mu_now, co, mo)
                    out["blocks_agree"] &= tm.same_bits(block(), ref)
                    fs.begin(state, g, sol, dirs[0], f, w[:8], alpha, mu_now)
                    while True:
                        for _k in range(rungs):
                            fs.trial(state, sol, dirs[0], xt, st)
                            model.obj_device(xt, out=ft)
                            model.cons(xt, ct)
                            bar.merit(xt, st, ct, out=mt)
                            fs.accept(ft, mt, mu_now, alpha)
                        sstate = fs.state()
                        if sstate["status"] != 0:
                            break
                    sname = sstate["status_name"]
                    if sname.startswith("accepted"):
                        break
                    dw = 1e-4 if dw == 0.0 else dw * 10.0
                if not sname.startswith("accepted"):
                    return False
                bar.update(state, sol, dirs, alpha, mu_now)
                evaluate()
                return True

            evaluate()
            s = None
            for it in range(limit):
                s = check()
                out["iterations"] = it
                if s["status"] != cref.ITERATING or not direction():
                    break
            out.update(status=s["status"], checks=s["checks"], state=s, block=block(), ref_block=ref.copy(), final=host(state), kept=host(conv.kept()))
            poisoned = tuple(torch.full_like(t, float("nan")) for t in state)
            out["restored"] = host(conv.restore(poisoned))
            for _ in range(past_latch):
                moved = direction()
                check()
                out["moved_past_latch"].append(moved)
            if past_latch:
                out.update(block_past_latch=block(), kept_past_latch=host(conv.kept()), final_past_latch=host(state))
            return out
        finally:
            fs.bind_mu(None)
            bar.bind_mu(None)
