"""numpy restatement of csrc/iem_rmu_device.h — the candidate ladder, the 32 words of rmu_error, rmu_update, rmu_enter and rmu_trigger,
expression for expression (numpy rounds every operation and contracts nothing: what -ffp-contract=off makes of the kernels) — on top
of tests/resto_reference.py, tests/mu_reference.py and tests/search_reference.py, and the host loop of resto_reference with the
restated rule, the STATIONARY exit and the trigger.  TEST INFRASTRUCTURE: tests/test_rmu.py (CPU), tests/test_gpu_rmu.py,
tests/rmu_loop.py.

The own block is a float64 array of sixteen words (words 0–3, 9, 10 hold int64 bit patterns: ``ints(blk)``), the restoration block is
mu_reference's, a search's control block search_reference's."""
import math

import numpy as np

import barrier_reference as bref
import mu_reference as mref
import resto_reference as rref
import search_reference as sref

K = 6
ITERATING, STATIONARY, UNUSABLE = 0, 1, 2
STATUS, FLAGS, LAST, TOTAL, E0, EMU, MU_ENTER, INF_ENTER, ALPHA_MIN, TRIG_ORIG, TRIG_INNER = range(11)
OPTS = dict(kappa_eps=10.0, kappa_mu=0.2, tau_min=0.99, tol=1e-8, mu_floor=1e-11, s_max=100.0, gamma_alpha=0.05)
F = np.float64
NAN = float("nan")


def ints(blk):
    return blk.view(np.int64)


def next_mu(mu, opts=OPTS):
    with np.errstate(all="ignore"):
        return np.maximum(F(opts["mu_floor"]), np.minimum(F(opts["kappa_mu"]) * mu, mu * np.sqrt(mu)))


def ladder(mblk, opts=OPTS):
    """the K candidates ``(mu_k, zeta_k)``: words 0 and 2 of the restoration block, then the monotone rule"""
    mu, zeta = [F(mblk[0])], [F(mblk[2])]
    for _ in range(1, K):
        mu.append(next_mu(mu[-1], opts))
        with np.errstate(all="ignore"):
            zeta.append(np.sqrt(mu[-1]))
    return np.array(mu), np.array(zeta)


def products(B, R, st):
    """the complementarity products of the restoration problem, each rounded once: the present bounds, then p·zp and n·zn on every row"""
    with np.errstate(all="ignore"):
        return np.concatenate([mref.products(B, st), R["p"] * R["zp"], R["n"] * R["zn"]])


def product_addends(B, R, st):
    """the products over [0, nvar + ncon) in rmu_error's statement order — lower then upper on a variable and on an inequality row,
    then p·zp, then n·zn on every row — and the masks of the present ones"""
    (pL, pU), (onL, onU) = mref.product_addends(B, st)
    every = np.ones(len(st[2]), dtype=bool)
    on_rows = np.concatenate([np.zeros(len(st[0]), dtype=bool), every])
    with np.errstate(all="ignore"):
        return ((pL, pU, bref.full(B, None, None, every, R["p"] * R["zp"]), bref.full(B, None, None, every, R["n"] * R["zn"])), (onL, onU, on_rows, on_rows))


def _words(B, R, st, r, c, mblk, opts, ropts, sums):
    """the 32 words, words 4–7, 9, 10 from `sums` (six numbers)"""
    mu, zeta = ladder(mblk, opts)
    w = np.zeros(32)
    head = rref.error(B, R, st, r, c, 0.0, float(zeta[0]), ropts)[0]
    w[0:4] = head
    w[4:8] = sums[:4]
    p = products(B, R, st)
    ok = mref.enters(np.ascontiguousarray(p))
    w[8] = float(p[ok].min()) if ok.any() else float("inf")
    w[9], w[10] = sums[4], sums[5]
    for k in range(K):
        hk = rref.error(B, R, st, r, c, 0.0, float(zeta[k]), ropts)[0]
        w[12 + 3 * k], w[13 + 3 * k], w[14 + 3 * k] = mu[k], hk[0], hk[1]
    return w


def error_words(B, R, st, r, c, mblk, opts=OPTS, ropts=rref.OPTS):
    """rmu_error with numpy's sums (the host loop's)"""
    _, ay, mult, theta, logs = rref.error(B, R, st, r, c, 0.0, float(mblk[2]), ropts)
    p = products(B, R, st)
    bad = float((~mref.enters(np.ascontiguousarray(p))).sum())
    with np.errstate(all="ignore"):
        sums = [float(ay.sum()), float(mult.sum()), float(theta.sum()), float(logs.sum()), float(p.sum()), bad]
    return _words(B, R, st, r, c, mblk, opts, ropts, sums)


def error_device(B, R, st, r, c, mblk, n_wg, opts=OPTS, ropts=rref.OPTS):
    """rmu_error on a grid of `n_wg` workgroups: every word carries the device's bits but [7], which is the device's order over numpy's
    logs"""
    sums = list(rref.error_sums(B, R, st, c, n_wg))
    addends, on = product_addends(B, R, st)
    bad = [np.where(o, ~mref.enters(np.ascontiguousarray(a)), False).astype(np.float64) for a, o in zip(addends, on)]
    sums += [bref.device_sum(list(addends), n_wg), bref.device_sum(bad, n_wg)]
    return _words(B, R, st, r, c, mblk, opts, ropts, sums)


def E(w, k, mu, counts, opts=OPTS):
    """E_k(mu) of rmu_update from the 32 words; counts = (ncon, nz + 2·ncon)"""
    m, nzr = int(counts[0]), int(counts[1])
    w = np.asarray(w, dtype=np.float64)
    s_max = F(opts["s_max"])
    with np.errstate(all="ignore"):
        sd = np.maximum(s_max, (w[4] + w[5]) / F(max(1, m + nzr))) / s_max
        sc = np.maximum(s_max, w[5] / F(max(1, nzr))) / s_max
        e_d = np.maximum(w[13 + 3 * k], w[14 + 3 * k]) / sd
        e_p = w[2] if m else F(0.0)
        e_c = np.maximum(w[3] - F(mu), F(mu) - w[8]) / sc if nzr else F(0.0)
        return np.maximum(np.maximum(e_d, e_p), e_c)


def update(own, mblk, ictl, w, counts, opts=OPTS):
    """rmu_update: ``(own block, restoration block, inner control block)`` after the call"""
    own, mblk, ictl = own.copy(), mblk.copy(), ictl.copy()
    w = np.asarray(w, dtype=np.float64)
    floor, kappa_eps = F(opts["mu_floor"]), F(opts["kappa_eps"])
    e0 = E(w, 0, 0.0, counts, opts)
    j, truncated = 0, 0
    solved = lambda k: bool(w[12 + 3 * k] > floor and E(w, k, w[12 + 3 * k], counts, opts) <= kappa_eps * w[12 + 3 * k])
    if w[10] != 0.0 or np.isnan(e0):
        status = UNUSABLE
    elif e0 <= opts["tol"]:
        status = STATIONARY
    else:
        status = ITERATING
        while j < K - 1 and solved(j):
            j += 1
        if j == K - 1 and solved(j):
            truncated = 2
    mu = F(w[12 + 3 * j])
    if j > 0:
        with np.errstate(all="ignore"):
            mblk[0], mblk[1], mblk[2] = mu, np.maximum(F(opts["tau_min"]), F(1.0) - mu), np.sqrt(mu)
        ictl[sref.COUNT] = ictl[sref.FLAGS] = 0.0
    iw = ints(own)
    iw[STATUS], iw[FLAGS], iw[LAST] = status, (1 if j > 0 else 0) | truncated, j
    iw[TOTAL] += j
    own[E0], own[EMU] = e0, E(w, j, mu, counts, opts)
    return own, mblk, ictl


def enter(own, mblk, ictl, err, mu_host, oblk=None, opts=OPTS):
    """rmu_enter: ``(own block, restoration block, inner control block)`` after the call"""
    own, mblk, ictl = own.copy(), mblk.copy(), ictl.copy()
    mu_orig = F(oblk[0]) if oblk is not None else F(mu_host)
    inf = F(err[2])
    with np.errstate(all="ignore"):
        mu_r = np.maximum(mu_orig, inf)
    if not mu_r > 0.0:
        ints(own)[STATUS] = UNUSABLE
        return own, mblk, ictl
    mblk = mref.reset(mblk, dict(opts, mu_init=0.1), mu_r)
    own[:] = 0.0
    own[MU_ENTER], own[INF_ENTER] = mu_r, inf
    ictl[sref.COUNT] = ictl[sref.FLAGS] = 0.0
    return own, mblk, ictl


def alpha_min(ctl, opts=OPTS, sopts=sref.OPTS):
    """Ipopt's alpha_min from words 3, 4, 5 of a control block, each operation rounded once"""
    theta0, slope, theta_min = F(ctl[sref.THETA0]), F(ctl[sref.SLOPE]), F(ctl[sref.THETA_MIN])
    a = F(sopts["gamma_theta"])
    with np.errstate(all="ignore"):
        if slope < 0.0:
            a = np.minimum(a, (F(sopts["gamma_phi"]) * theta0) / (-slope))
        if slope < 0.0 and theta0 <= theta_min:
            a = np.minimum(a, (F(sopts["delta"]) * np.power(theta0, F(sopts["s_theta"]))) / np.power(-slope, F(sopts["s_phi"])))
        return F(opts["gamma_alpha"]) * a


def trigger(own, ctl, which, opts=OPTS, sopts=sref.OPTS):
    """rmu_trigger: ``(own block, control block, d_alpha[0] or None where it is not written)``"""
    own, ctl = own.copy(), ctl.copy()
    if sref.word(ctl, sref.STATUS) != sref.SEARCHING:
        return own, ctl, None
    amin = alpha_min(ctl, opts, sopts)
    own[ALPHA_MIN] = amin
    if ctl[sref.ALPHA] < amin:
        sref.set_word(ctl, sref.STATUS, sref.FAILED)
        ctl[sref.ALPHA] = 0.0
        ints(own)[TRIG_INNER if which else TRIG_ORIG] += 1
        return own, ctl, 0.0
    return own, ctl, None


def fresh_own():
    return np.zeros(16)


# ---- the host loop: resto_reference.host_loop with the restated rule, the STATIONARY exit and the trigger ------------------------------
def host_restoration(om, B, st, mu_orig, ctl_o, filt_o, own, opts=OPTS, ropts=rref.OPTS, sopts=sref.OPTS, max_iter=100, use_trigger=True, stats=None, log=None):
    """resto_reference.host_restoration with `update` deciding mu, STATIONARY / UNUSABLE ending the phase, and `trigger` behind every
    accept of the inner search.  ``(state or None, iterations, ORIGINAL block, ORIGINAL filter, why, own block)``"""
    n_, m = om.nvar, om.ncon
    c = om.cons(st[0])
    with np.errstate(invalid="ignore"):
        inf = float(np.abs(rref.infeasibility(B, c, st[1])).max())
    ictl, filt = sref.block(status=sref.UNUSABLE), np.zeros((sopts["filter_capacity"], 2))
    own, mblk, ictl = enter(own, mref.fresh_block(dict(opts, mu_init=0.1)), ictl, np.array([0.0, 0.0, inf, 0, 0, 0, 0, 0]), mu_orig, None, opts)
    if ints(own)[STATUS] == UNUSABLE:
        return None, 0, ctl_o, filt_o, "unusable", own
    R, st = rref.enter(B, rref.new_object(n_, m), st, c, float(mblk[0]), ropts)
    R["blk"], ctl_o, filt_o = rref.enter_filter(R["blk"], ctl_o, filt_o, sopts)
    counts = (m, B["counts"]["nz"] + 2 * m)
    nanc = np.full(m, NAN)
    for it in range(max_iter):
        x, s, y = st[0], st[1], st[2]
        c = om.cons(x)
        r = om.jtprod(x, y)
        w = error_words(B, R, st, r, c, mblk, opts, ropts)
        own, mblk, ictl_new = update(own, mblk, ictl, w, counts, opts)
        if stats is not None:
            stats["decreases"].append(int(ints(own)[LAST]))
            stats["truncated"] = stats["truncated"] or bool(ints(own)[FLAGS] & 2)
            stats["e0"].append(float(own[E0]))
        if ints(own)[FLAGS] & 1:
            ictl, filt = ictl_new, np.zeros((sopts["filter_capacity"], 2))
        if ints(own)[STATUS] == STATIONARY:
            return None, it + 1, ctl_o, filt_o, "stationary", own
        if ints(own)[STATUS] == UNUSABLE:
            return None, it + 1, ctl_o, filt_o, "unusable", own
        mu, tau, zeta = float(mblk[0]), float(mblk[1]), float(mblk[2])
        sigma, dcon, rhs = rref.terms(B, R, st, r, c, mu, zeta, ropts)
        W, J = rref._matrices(om, x, y, 0.0)
        sol, dw = rref._solve_K(W, J, sigma, dcon, 0.0, rhs, m)
        dirs, alpha, R = rref.step(B, R, st, sol, (nanc, nanc, nanc), mu, tau, zeta, ropts)
        m0 = rref.merit(B, R, 0, x, s, c, zeta, ropts)
        ictl = rref.begin(ictl, float(rref.slope_terms(B, R, st, sol, dirs[0], mu, zeta, ropts).sum()), m0, alpha, mu)
        d_alpha = alpha.copy()
        while sref.word(ictl, sref.STATUS) == sref.SEARCHING:
            xt, s_t, R = rref.trial(B, R, ictl, x, s, sol, dirs[0], (x, s))
            mt = rref.merit(B, R, 1, xt, s_t, om.cons(xt), zeta, ropts)
            ictl, filt, d_alpha[0] = sref.accept(ictl, filt, mt[0], mt[1:], mu, 1.0, sopts)
            if stats is not None:
                stats["accepts"] += 1
            if use_trigger:
                own, ictl, a0 = trigger(own, ictl, 1, opts, sopts)
                d_alpha[0] = d_alpha[0] if a0 is None else a0
        if sref.word(ictl, sref.STATUS) not in (sref.F_TYPE, sref.H_TYPE):
            return None, it + 1, ctl_o, filt_o, "inner search failed", own
        st, R = rref.update(B, R, st, sol, dirs, d_alpha, mu)
        c = om.cons(st[0])
        theta, logs = bref.merit_terms(B, st[0], st[1], c)
        R["blk"] = rref.check(R["blk"], ctl_o, filt_o, om.obj(st[0]), np.array([float(theta.sum()), float(logs.sum())]), mu_orig, ropts, sopts["filter_capacity"])
        if log:
            log(dict(resto_iter=it, mu=mu, alpha=float(d_alpha[0]), theta=float(R["blk"][rref.R_THETA]), dw=dw))
        if int(R["blk"].view(np.int64)[rref.R_STATE]) == rref.RETURN:
            st, _ = rref.leave(B, R["blk"], st, ropts)
            return st, it + 1, ctl_o, filt_o, "returned", own
    return None, max_iter, ctl_o, filt_o, "no return within the cap", own


def host_loop(om, x0=None, max_restorations=5, tol=1e-8, max_iter=200, mu=0.1, opts=OPTS, ropts=rref.OPTS, sopts=sref.OPTS, use_trigger=True, log=None):
    """resto_reference.host_loop with the trigger behind every accept of the original search and `host_restoration` above as the phase.
    Returns its dict with ``status`` also "locally infeasible" (the restoration ended STATIONARY), ``accepts`` (calls of accept, both
    searches), ``decreases`` (per restoration update), ``truncated``, ``triggers`` (original, inner), ``iterates`` (x per iteration)."""
    B = bref.relaxed_bounds(om.lvar, om.uvar, om.lcon, om.ucon, bref.RELAX)
    m = om.ncon
    nanc = np.full(m, NAN)
    x = np.array(om.x0 if x0 is None else x0, dtype=np.float64)
    x, s, zL, zU, vL, vU = bref.start(B, x, om.cons(x), (nanc, nanc, nanc))
    st = (x, s, np.zeros(m), zL, zU, vL, vU)
    ctl, filt = sref.block(status=sref.UNUSABLE), np.zeros((sopts["filter_capacity"], 2))
    counts = (m, B["counts"]["nz"])
    mu_floor = max(1e-11, tol / 10.0)
    stats = dict(accepts=0, decreases=[], truncated=False, e0=[])
    own = fresh_own()
    out = dict(restorations=0, resto_iterations=0, why=None, iterates=[])

    def done(status):
        out.update(status=status, accepts=stats["accepts"], decreases=stats["decreases"], truncated=stats["truncated"], e0=stats["e0"],
                   triggers=(int(ints(own)[TRIG_ORIG]) + out.get("_trig_orig", 0), out.get("_trig_inner", 0) + int(ints(own)[TRIG_INNER])))
        return out

    for it in range(max_iter + 1):
        x, s, y = st[0], st[1], st[2]
        c, g = om.cons(x), om.grad(x)
        r = g + om.jtprod(x, y)
        head, ay, mult, theta, logs = bref.error(B, st, r, c, 0.0)
        err = rref._opt_err(head, (float(ay.sum()), float(mult.sum())), counts)
        out.update(iterations=it, error=err, x=x, objective=float(om.obj(x)))
        out["iterates"].append(x.copy())
        if err <= tol or it == max_iter:
            return done("solved" if err <= tol else "max_iter")
        changed = False
        while mu > mu_floor:
            head, ay, mult, _, _ = bref.error(B, st, r, c, mu)
            if rref._opt_err(head, (float(ay.sum()), float(mult.sum())), counts) > rref.KAPPA_EPS * mu:
                break
            mu, changed = max(mu_floor, min(rref.KAPPA_MU * mu, mu ** rref.THETA_MU)), True
        if changed:
            ctl, filt = sref.block(status=sref.UNUSABLE), np.zeros((sopts["filter_capacity"], 2))
        tau = max(rref.TAU_MIN, 1.0 - mu)
        sigma, dcon, rhs = bref.terms(B, st, r, c, mu)
        W, J = rref._matrices(om, x, y, 1.0)
        dw, ok = 0.0, False
        for _ in range(8):
            sol, dw = rref._solve_K(W, J, sigma, dcon, dw, rhs, m)
            dirs, alpha = bref.step(B, st, sol, (nanc, nanc, nanc), mu, tau)
            slope = float(sref.slope_terms(B, x, s, g, sol, dirs[0], mu).sum())
            ctl = sref.begin(ctl, slope, om.obj(x), np.array([0, 0, 0, 0, 0, 0, float(theta.sum()), float(logs.sum())]), alpha, mu)
            d_alpha = alpha.copy()
            while sref.word(ctl, sref.STATUS) == sref.SEARCHING:
                xt, s_t = sref.trial(B, ctl, x, s, sol, dirs[0], (x, s))
                th_t, lg_t = bref.merit_terms(B, xt, s_t, om.cons(xt))
                ctl, filt, d_alpha[0] = sref.accept(ctl, filt, om.obj(xt), np.array([float(th_t.sum()), float(lg_t.sum())]), mu, 1.0, sopts)
                stats["accepts"] += 1
                if use_trigger:
                    own, ctl, a0 = trigger(own, ctl, 0, opts, sopts)
                    d_alpha[0] = d_alpha[0] if a0 is None else a0
            if sref.word(ctl, sref.STATUS) in (sref.F_TYPE, sref.H_TYPE):
                ok = True
                break
            dw = 1e-4 if dw == 0.0 else dw * 10.0
        if log:
            log(dict(iter=it, error=err, mu=mu, objective=out["objective"], theta=float(theta.sum()), alpha=float(d_alpha[0]), status=sref.word(ctl, sref.STATUS)))
        if ok:
            st = bref.update(B, st, sol, dirs, d_alpha, mu)
            continue
        if out["restorations"] >= max_restorations:
            return done("search failed")
        # (enter zeroes the own block: the triggers counted so far are carried over)
        out["_trig_orig"] = out.get("_trig_orig", 0) + int(ints(own)[TRIG_ORIG])
        out["_trig_inner"] = out.get("_trig_inner", 0) + int(ints(own)[TRIG_INNER])
        new, k, ctl, filt, why, own = host_restoration(om, B, st, mu, ctl, filt, own, opts, ropts, sopts, use_trigger=use_trigger, stats=stats, log=log)
        out["resto_iterations"] += k
        out["why"] = why
        if new is None:
            return done("locally infeasible" if why == "stationary" else "restoration failed")
        out["restorations"] += 1
        st = new
    return done("max_iter")
