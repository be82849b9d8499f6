"""numpy restatement of csrc/iem_mpc_device.h — mpc_terms, mpc_step and the decision and copy of mpc_select, expression for expression
(numpy rounds every operation and contracts nothing: what -ffp-contract=off makes of the kernels) — on top of
tests/barrier_reference.py, tests/mu_reference.py and tests/amu_reference.py.  TEST INFRASTRUCTURE: tests/test_mpc.py (CPU),
tests/test_gpu_mpc.py, tests/mpc_loop.py.

The own block: sixteen float64 words, words 0–2, 5, 6 as bit patterns (``ints(blk)`` is the int64 view).  Where the kernels branch on a
presence flag the restatement computes on every entry and selects with np.where, as barrier_reference does."""
import numpy as np

import amu_reference as aref
import barrier_reference as bref
import mu_reference as mref

OPTS = dict(red_fact=1.0)
F = np.float64
ints = mref.ints
TAKEN, N_TAKEN, N_REFUSED, PREDICTED, AVG, ALPHA_P, ALPHA_D = range(7)
REASONS = ("taken", "nz = 0", "NaN product", "zero step length", "average")


def options(**over):
    return {**OPTS, **over}


def fresh_block():
    """the own block behind iem_mpc_create / iem_mpc_reset"""
    return np.zeros(16)


def targets(B, sol_a, dirs_a, mu):
    """the per-bound targets in the place of mu: ``(mL, mU, nL, nU)`` — lower: mu − d_aff·dz_aff, upper: mu + d_aff·dz_aff (its gap
    moves by −d), d_aff = dx_aff on variables and ds_aff on rows"""
    ds, dzL, dzU, dvL, dvU = dirs_a
    dx = np.asarray(sol_a)[:len(B["hasL"])]
    mu = F(mu)
    with np.errstate(all="ignore"):
        return mu - dx * dzL, mu + dx * dzU, mu - ds * dvL, mu + ds * dvU


def _side(B, st, m4):
    """barrier_reference._side with a target per bound"""
    x, s, y, zL, zU, vL, vU = st
    mL, mU, nL, nU = m4
    with np.errstate(all="ignore"):
        dL, dU, eL, eU = x - B["xl"], B["xu"] - x, s - B["rl"], B["ru"] - s
        q = dict(dL=dL, dU=dU, eL=eL, eU=eU)
        q["sl"], q["su"] = np.where(B["hasL"], zL / dL, 0.0), np.where(B["hasU"], zU / dU, 0.0)
        q["ml"], q["mu"] = np.where(B["hasL"], mL / dL, 0.0), np.where(B["hasU"], mU / dU, 0.0)
        q["tl"], q["tu"] = np.where(B["gL"], vL / eL, 0.0), np.where(B["gU"], vU / eU, 0.0)
        q["nl"], q["nu"] = np.where(B["gL"], nL / eL, 0.0), np.where(B["gU"], nU / eU, 0.0)
        q["sigs"] = q["tl"] + q["tu"]
        q["rs"] = (q["nu"] - q["nl"]) - y
    return q


def _rhs(B, st, r, c, q):
    with np.errstate(all="ignore"):
        rhs_x = -(r + (q["mu"] - q["ml"]))
        inv = 1.0 / q["sigs"]
        rhs_y = np.where(B["eq"], -(c - B["ceq"]), -((c - st[1]) + q["rs"] * inv))
    return np.concatenate([rhs_x, rhs_y])


def terms(B, st, r, c, sol_a, dirs_a, mu):
    """``(column 0, column 1)`` of mpc_terms: column 0 is barrier_reference.terms(...)[2] at that mu"""
    return bref.terms(B, st, r, c, mu)[2], _rhs(B, st, r, c, _side(B, st, targets(B, sol_a, dirs_a, mu)))


def step(B, st, sol_a, dirs_a, sol, bufs, mu, tau):
    """mpc_step: ``((ds, dzL, dzU, dvL, dvU), alpha)`` of the corrected solution `sol`; bufs = (ds, dvL, dvU) as they were: entries on
    equality rows stay.  barrier_reference.step with the targets in the place of mu"""
    x, s, y, zL, zU, vL, vU = st
    nvar = len(x)
    dx, dy = sol[:nvar], sol[nvar:]
    q = _side(B, st, targets(B, sol_a, dirs_a, mu))
    ine = ~B["eq"]
    tau = F(tau)
    with np.errstate(all="ignore"):
        ds_all = (dy - q["rs"]) / q["sigs"]
        dzL = np.where(B["hasL"], (q["ml"] - zL) - q["sl"] * dx, 0.0)
        dzU = np.where(B["hasU"], (q["mu"] - zU) + q["su"] * dx, 0.0)
        dvL_all = np.where(B["gL"], (q["nl"] - vL) - q["tl"] * ds_all, 0.0)
        dvU_all = np.where(B["gU"], (q["nu"] - vU) + q["tu"] * ds_all, 0.0)
        ap = bref._alpha([(((-tau) * q["dL"]) / dx, B["hasL"] & (dx < 0)), ((tau * q["dU"]) / dx, B["hasU"] & (dx > 0)),
                          (((-tau) * q["eL"]) / ds_all, B["gL"] & (ds_all < 0)), ((tau * q["eU"]) / ds_all, B["gU"] & (ds_all > 0))])
        ad = bref._alpha([(((-tau) * zL) / dzL, B["hasL"] & (dzL < 0)), (((-tau) * zU) / dzU, B["hasU"] & (dzU < 0)),
                          (((-tau) * vL) / dvL_all, B["gL"] & (dvL_all < 0)), (((-tau) * vU) / dvU_all, B["gU"] & (dvU_all < 0))])
        if np.isnan(sol).any() or np.isnan(ds_all[ine]).any():
            ap = 0.0
        if np.isnan(dzL[B["hasL"]]).any() or np.isnan(dzU[B["hasU"]]).any() or np.isnan(dvL_all[B["gL"]]).any() or np.isnan(dvU_all[B["gU"]]).any():
            ad = 0.0
    dirs = (np.where(ine, ds_all, bufs[0]), dzL, dzU, np.where(ine, dvL_all, bufs[1]), np.where(ine, dvU_all, bufs[2]))
    return dirs, np.array([ap, ad])


def decide(probe, alpha_c, avg, nz, opts):
    """the decision of mpc_select: ``(taken, predicted, reason)`` — reason names the first condition that refuses (REASONS)"""
    q = np.asarray(probe, dtype=np.float64)
    a = np.asarray(alpha_c, dtype=np.float64)
    nz = int(nz)
    with np.errstate(all="ignore"):
        predicted = q[0] / F(nz) if nz else F(0.0)
        bound = F(opts["red_fact"]) * F(avg)
        if nz == 0:
            reason = 1
        elif not q[1] == 0.0:
            reason = 2
        elif a[0].view(np.int64) == 0 or a[1].view(np.int64) == 0:
            reason = 3
        elif not predicted <= bound:      # a NaN compares false
            reason = 4
        else:
            reason = 0
    return reason == 0, F(predicted), REASONS[reason]


def select(B, blk, probe, alpha_c, ab, opts, corrected, first, alpha):
    """mpc_select: ``(own block, first-order (sol, ds, dzL, dzU, dvL, dvU), alpha)`` after the call; `corrected` and `first` are
    (sol, ds, dzL, dzU, dvL, dvU).  Taken: sol whole, dzL, dzU whole, ds, dvL, dvU on inequality rows, and both words of alpha."""
    blk = blk.copy()
    nz = B["counts"]["nz"]
    avg = F(ab[aref.AVG])
    taken, predicted, _ = decide(probe, alpha_c, avg, nz, opts)
    iw = ints(blk)
    n_t, n_r = int(iw[N_TAKEN]), int(iw[N_REFUSED])
    blk[:] = 0.0
    iw[TAKEN], iw[N_TAKEN], iw[N_REFUSED] = int(taken), n_t + int(taken), n_r + int(not taken)
    blk[PREDICTED], blk[AVG] = predicted, avg
    blk[ALPHA_P], blk[ALPHA_D] = alpha_c[0], alpha_c[1]
    if not taken:
        return blk, tuple(first), np.asarray(alpha)
    ine = ~B["eq"]
    out = [corrected[0].copy(), np.where(ine, corrected[1], first[1]), corrected[2].copy(), corrected[3].copy(), np.where(ine, corrected[4], first[4]),
           np.where(ine, corrected[5], first[5])]
    return blk, tuple(out), np.array([alpha_c[0], alpha_c[1]])


def newton_blocks(P, K_parts, sol_a, dirs_a, sol, dirs, dw, dc, mu):
    """barrier_reference.newton_blocks for the CORRECTED direction: the same three linear blocks, and complementarity rows whose
    target is mu − dgap_aff·dz_aff per bound (dgap_aff = dx_aff, −dx_aff, ds_aff, −ds_aff for xL, xU, sL, sU)"""
    B = P["B"]
    x, s, y, zL, zU, vL, vU = P["state"]
    ds, dzL, dzU, dvL, dvU = dirs
    ds_a, dzL_a, dzU_a, dvL_a, dvU_a = dirs_a
    nvar = len(x)
    dx, dx_a = sol[:nvar], sol_a[:nvar]
    b1, b2, b3, _ = bref.newton_blocks(P, K_parts, sol, dirs, dw, dc, mu)
    with np.errstate(all="ignore"):
        tL, tU = mu - dx_a * dzL_a, mu - (-dx_a) * dzU_a
        uL, uU = mu - ds_a * dvL_a, mu - (-ds_a) * dvU_a
        b4 = np.concatenate([(zL * dx + (x - B["xl"]) * dzL - (tL - (x - B["xl"]) * zL))[B["hasL"]], (-zU * dx + (B["xu"] - x) * dzU - (tU - (B["xu"] - x) * zU))[B["hasU"]],
                             (vL * ds + (s - B["rl"]) * dvL - (uL - (s - B["rl"]) * vL))[B["gL"]], (-vU * ds + (B["ru"] - s) * dvU - (uU - (B["ru"] - s) * vU))[B["gU"]]])
    return b1, b2, b3, b4


def corrected(P, mu, dw=1e-2, tau=bref.TAU):
    """One iteration's directions at P's state on the host: the affine direction (terms at mu = 0, scipy's LU of
    kkt_diag_reference.host_kkt_diag, step at tau = 1), the two columns of `terms` at `mu`, both solves, barrier_reference.step on
    column 0 and `step` on column 1.  Returns dict(aff, first, corr: (sol, dirs, alpha); rhs: the two columns)."""
    import kkt_diag_reference as dref
    from scipy.sparse.linalg import splu
    B, st, om = P["B"], P["state"], P["om"]
    sigma, dcon, rhs_a = bref.terms(B, st, P["r"], P["c"], 0.0)
    lu = splu(dref.host_kkt_diag(om, st[0], st[2], sigma, dw, dcon + 0.0).tocsc())
    poison = lambda: tuple(np.full(om.ncon, bref.NAN) for _ in range(3))
    sol_a = lu.solve(rhs_a)
    dirs_a, alpha_a = bref.step(B, st, sol_a, poison(), 0.0, 1.0)
    rhs0, rhs1 = terms(B, st, P["r"], P["c"], sol_a, dirs_a, mu)
    sol0, sol1 = lu.solve(rhs0), lu.solve(rhs1)
    dirs0, alpha0 = bref.step(B, st, sol0, poison(), mu, tau)
    dirs1, alpha1 = step(B, st, sol_a, dirs_a, sol1, poison(), mu, tau)
    return dict(aff=(sol_a, dirs_a, alpha_a), first=(sol0, dirs0, alpha0), corr=(sol1, dirs1, alpha1), rhs=(rhs0, rhs1))


def host_loop(om, corrector=True, tol=1e-8, max_iter=200, mu=0.1, mpc_opts=None, log=None):
    """The probing rule (amu_reference) with — or, corrector = False, without — Mehrotra's corrector on the HOST alone, in the manner
    of qf_reference.host_loop: barrier_reference (start, terms, step, update, merit), mu_reference.error_words (sums in numpy's order),
    amu_reference (probe_words, update), the restatements above, search_reference, around a dense solve of the regularised KKT system
    whose inertia the eigenvalues give.  Per iteration: error, the affine direction and its probe, the rule's update, the two columns
    at the new mu, both solves, both steps, the probe of the corrected direction, the decision, the search on what it left.
    Returns dict(x, objective, iterations, error, status, failed, mus, taken, refused, reasons)."""
    import search_reference as sref
    from kkt_diag_reference import host_kkt_diag
    B = bref.relaxed_bounds(om.lvar, om.uvar, om.lcon, om.ucon, bref.RELAX)
    n, m = om.nvar, om.ncon
    counts = (B["counts"]["ncon"], B["counts"]["nz"])
    opts, aopts, mopts = mref.options(mu_init=mu, tol=tol), aref.options(), options(**(mpc_opts or {}))
    blk, ab, qb = mref.fresh_block(opts), aref.fresh_block(aopts), fresh_block()
    zero = lambda: tuple(np.zeros(m) for _ in range(3))
    x = np.array(om.x0, dtype=np.float64)
    x, s, zL, zU, vL, vU = bref.start(B, x, om.cons(x), zero())
    y = np.zeros(m)
    ctl, filt = sref.block(status=sref.UNUSABLE), np.zeros((sref.OPTS["filter_capacity"], 2))
    out = dict(failed=0, mus=[], reasons=[], status=None, taken=0, refused=0)
    for it in range(max_iter + 1):
        st = (x, s, y, zL, zU, vL, vU)
        c, g, f = om.cons(x), om.grad(x), om.obj(x)
        r = g + om.jtprod(x, y)
        head, sums, w8, w10, p = mref.error_words(B, st, r, c)
        w = np.array([*head, *(float(np.sum(t)) for t in sums), w8, float(np.sum(p)), w10, 0.0])
        sigma, dcon, rhs_a = bref.terms(B, st, r, c, 0.0)
        state = dict(dw=0.0, tries=0, K=None)

        def factorise():
            while True:
                K = host_kkt_diag(om, x, y, sigma, state["dw"], dcon + 1e-10).toarray()
                state["tries"] += 1
                ev = np.linalg.eigvalsh(K)
                if int((ev < 0).sum()) == m or state["tries"] >= 24:
                    state["K"] = K
                    return
                state["dw"] = 1e-4 if state["dw"] == 0.0 else state["dw"] * (100.0 if state["tries"] <= 2 else 8.0)
        factorise()
        sol_a = np.linalg.solve(state["K"], rhs_a)
        dirs_a, alpha_a = bref.step(B, st, sol_a, zero(), 0.0, 1.0)
        pa = aref.probe_words(B, st, sol_a, dirs_a, alpha_a)
        blk, ab, _ = aref.update(blk, ab, w, np.array([float(np.sum(pa[0])), *pa[1:]]), counts, opts, aopts)
        iw = ints(blk)
        mu_k, tau, status = float(blk[0]), float(blk[1]), int(iw[8])
        if iw[9] & 1:
            sref.set_word(ctl, sref.COUNT, 0)
            sref.set_word(ctl, sref.FLAGS, 0)
        out.update(iterations=it, error=float(blk[3]), status=status)
        out["mus"].append(mu_k)
        if log:
            log(dict(iter=it, error=float(blk[3]), mu=mu_k, f=f, taken=out["taken"], refused=out["refused"]))
        if status != mref.ITERATING or it == max_iter:
            break
        accepted, factored = False, True
        for _ in range(8):
            if not factored:
                factorise()      # (the affine direction stays that of the iteration's first factors, as in tests/mpc_loop.py)
            factored = False
            rhs0, rhs1 = terms(B, st, r, c, sol_a, dirs_a, mu_k)
            sol = np.linalg.solve(state["K"], rhs0)
            dirs, alpha = bref.step(B, st, sol, zero(), mu_k, tau)
            if corrector:
                sol_c = np.linalg.solve(state["K"], rhs1)
                dirs_c, alpha_c = step(B, st, sol_a, dirs_a, sol_c, zero(), mu_k, tau)
                pc = aref.probe_words(B, st, sol_c, dirs_c, alpha_c)
                probe = np.array([float(np.sum(pc[0])), *pc[1:]])
                out["reasons"].append(decide(probe, alpha_c, ab[aref.AVG], counts[1], mopts)[2])
                qb, d1, alpha = select(B, qb, probe, alpha_c, ab, mopts, (sol_c, *dirs_c), (sol, *dirs), alpha)
                sol, dirs = d1[0], tuple(d1[1:])
                out["taken"], out["refused"] = int(ints(qb)[N_TAKEN]), int(ints(qb)[N_REFUSED])
            slope = float(np.sum(sref.slope_terms(B, x, s, g, sol, dirs[0], mu_k)))
            theta, logs = bref.merit_terms(B, x, s, c)
            err = np.array([0, 0, 0, 0, 0, 0, float(np.sum(theta)), float(np.sum(logs))])
            ctl = sref.begin(ctl, slope, f, err, alpha, mu_k)
            while sref.word(ctl, sref.STATUS) == sref.SEARCHING:
                xt, s_t = sref.trial(B, ctl, x, s, sol, dirs[0], (x, s))
                ct = om.cons(xt)
                theta_t, logs_t = bref.merit_terms(B, xt, s_t, ct)
                ctl, filt, a = sref.accept(ctl, filt, om.obj(xt), np.array([float(np.sum(theta_t)), float(np.sum(logs_t))]), mu_k)
            if sref.word(ctl, sref.STATUS) in (sref.F_TYPE, sref.H_TYPE):
                accepted = True
                break
            out["failed"] += 1
            state["dw"] = 1e-4 if state["dw"] == 0.0 else state["dw"] * 10.0
        if not accepted:
            break
        x, s, y, zL, zU, vL, vU = bref.update(B, st, sol, dirs, np.array([a, alpha[1]]), mu_k)
    out.update(x=x, objective=float(om.obj(x)))
    return out
