"""numpy restatement of csrc/iem_qf_device.h — qf_begin, qf_alpha, qf_value and qf_update blocks in, blocks out, expression for
expression (numpy rounds every operation and contracts nothing: what -ffp-contract=off makes of the kernels) — on top of
tests/amu_reference.py, tests/mu_reference.py and tests/barrier_reference.py.  TEST INFRASTRUCTURE: tests/test_qf.py (CPU),
tests/test_gpu_qf.py, tests/qf_loop.py.

THE SUMS are restated in the device's order (`device_sum`): a lane adds the addends of its entries i, i + 256·n_wg, ... one after the
other from +0.0, the 64 lanes of a wave meet in the shuffle tree of iem_wave_sum, the four waves of a workgroup are added in order,
and the last arrival totals the column — lane l takes the workgroups l, l + 64, ..., then the same tree.  So `begin` and `value` are
bitwise the kernels for the grid (`n_wg` workgroups) they are given.

Three blocks: the iem_mu block and the iem_amu block (sixteen float64 words each, amu_reference / mu_reference) and the object's
own of thirty-two — words 0–3 hold int64 bit patterns, words 5 and 6 the alpha slots (`ints(blk)` is the int64 view)."""
import numpy as np

import amu_reference as aref
import barrier_reference as bref
import mu_reference as mref

IDLE, SECTION, DONE, UNUSABLE = 0, 1, 2, 3
OPTS = dict(mu_ref=1.0, sigma_min=1e-6, sigma_max=0.0, section_sigma_tol=1e-2, max_section_steps=8)
GOLDEN = 0.6180339887498949
F = np.float64
INF = F(np.inf)
ints = mref.ints
# the own block's words
(STATUS, PHASE, STEPS, EVALS, SIGMA, ALPHA_P, ALPHA_D, D2, P2, AVG, LO, HI, A_, B_, C_, D_, QC, QD, BEST, QBEST, Q0, Q, C2, NANS, LAST_AP, LAST_AD,
 SIGMA0) = range(27)
WORDS = 32
FIRST, SECOND, LEFT, RIGHT, NEW_LEFT, NEW_RIGHT = range(6)


def options(aopts=None, **over):
    """the options as iem_qf_create resolves them: sigma_max = 0 becomes the iem_amu object's"""
    o = {**OPTS, **over}
    if o["sigma_max"] == 0.0:
        o["sigma_max"] = (aopts if aopts is not None else aref.OPTS)["sigma_max"]
    return o


def fresh_block():
    """the own block behind iem_qf_create / iem_qf_reset"""
    return np.zeros(WORDS)


device_sum, _tree, _full = bref.device_sum, bref._tree, bref.full      # (the sums in the device's order live with the barrier layer's restatement)


def begin(B, st, r, c, w, ab, aopts, qopts, n_wg):
    """qf_begin: the own block after the call"""
    x, s, y, zL, zU, vL, vU = st
    ine = ~B["eq"]
    nz = int(B["counts"]["nz"])
    with np.errstate(all="ignore"):
        t = np.asarray(r, dtype=np.float64)
        t = np.where(B["hasL"], t - zL, t)
        t = np.where(B["hasU"], t + zU, t)
        u = -y
        u = np.where(B["gL"], u - vL, u)
        u = np.where(B["gU"], u + vU, u)
        inf = np.where(B["eq"], c - B["ceq"], c - s)
        allx = np.ones(len(x), dtype=bool)
        d2 = device_sum([_full(B, allx, t * t, ine, u * u)], n_wg)
        p2 = device_sum([_full(B, ~allx, t, np.ones(len(y), dtype=bool), inf * inf)], n_wg)
        q = fresh_block()
        q[D2], q[P2] = d2, p2
        if nz == 0:
            ints(q)[STATUS] = DONE
            return q
        avg = F(w[9]) / F(nz)
        mu_hi = F(ab[aref.MU_MAX])
        if mu_hi.view(np.int64) == 0:
            mu_hi = F(aopts["mu_max_fact"]) * avg
        lo = np.maximum(F(qopts["sigma_min"]), F(aopts["mu_min"]) / avg)
        hi = np.maximum(lo, np.minimum(F(qopts["sigma_max"]), mu_hi / avg))
        first = np.minimum(np.maximum(F(1.0), lo), hi)
    q[AVG], q[LO], q[HI], q[SIGMA], q[SIGMA0] = avg, lo, hi, first, first
    q[ALPHA_P] = q[ALPHA_D] = 1.0
    ints(q)[PHASE], ints(q)[STATUS] = FIRST, SECTION
    return q


def scale(qb, qopts):
    """t = (sigma·avg)/mu_ref of the trial sigma"""
    with np.errstate(all="ignore"):
        t = F(qb[SIGMA]) * F(qb[AVG])
        return t / F(qopts["mu_ref"])


def direction(d0, d1, t):
    """THE combination, per component: e = d1 − d0; u = t·e; d = d0 + u"""
    with np.errstate(all="ignore"):
        out = []
        for a0, a1 in zip(d0, d1):
            e = np.asarray(a1, dtype=np.float64) - np.asarray(a0, dtype=np.float64)
            out.append(a0 + t * e)
        return tuple(out)


def step_lengths(B, st, d, tau):
    """the two minima of qf_alpha for the direction d = (sol, ds, dzL, dzU, dvL, dvU): barrier_reference.step's candidates and rules,
    dy not read"""
    x, s, y, zL, zU, vL, vU = st
    sol, ds, dzL, dzU, dvL, dvU = d
    nvar = len(x)
    dx = np.asarray(sol)[:nvar]
    ine = ~B["eq"]
    tau = F(tau)
    with np.errstate(all="ignore"):
        dL, dU, eL, eU = x - B["xl"], B["xu"] - x, s - B["rl"], B["ru"] - s
        ap = bref._alpha([(((-tau) * dL) / dx, B["hasL"] & (dx < 0)), ((tau * dU) / dx, B["hasU"] & (dx > 0)),
                          (((-tau) * eL) / ds, B["gL"] & (ds < 0)), ((tau * eU) / ds, B["gU"] & (ds > 0))])
        ad = bref._alpha([(((-tau) * zL) / dzL, B["hasL"] & (dzL < 0)), (((-tau) * zU) / dzU, B["hasU"] & (dzU < 0)),
                          (((-tau) * vL) / dvL, B["gL"] & (dvL < 0)), (((-tau) * vU) / dvU, B["gU"] & (dvU < 0))])
        if np.isnan(dx).any() or np.isnan(ds[ine]).any():
            ap = 0.0
        if np.isnan(dzL[B["hasL"]]).any() or np.isnan(dzU[B["hasU"]]).any() or np.isnan(dvL[B["gL"]]).any() or np.isnan(dvU[B["gU"]]).any():
            ad = 0.0
    return F(ap), F(ad)


def alpha(B, st, d0, d1, qb, blk, qopts):
    """qf_alpha: the own block after the call (the two slots only); nothing unless a section is open"""
    qb = qb.copy()
    if ints(qb)[STATUS] != SECTION:
        return qb
    ap, ad = step_lengths(B, st, direction(d0, d1, scale(qb, qopts)), blk[1])
    qb[ALPHA_P], qb[ALPHA_D] = min(F(qb[ALPHA_P]), ap), min(F(qb[ALPHA_D]), ad)      # (non-negative doubles order like their bits)
    return qb


def products(B, st, d, ap, ad):
    """``(pL, pU)`` over [0, nvar + ncon) — the products of qf_value at the lower and the upper bounds in amu_probe's operation order,
    +0.0 where the bound is absent — and the masks"""
    x, s, y, zL, zU, vL, vU = st
    sol, ds, dzL, dzU, dvL, dvU = d
    dx = np.asarray(sol)[:len(x)]
    ap, ad = F(ap), F(ad)
    with np.errstate(all="ignore"):
        tx, ts = ap * dx, ap * ds
        pL = _full(B, B["hasL"], ((x - B["xl"]) + tx) * (zL + ad * dzL), B["gL"], ((s - B["rl"]) + ts) * (vL + ad * dvL))
        pU = _full(B, B["hasU"], ((B["xu"] - x) - tx) * (zU + ad * dzU), B["gU"], ((B["ru"] - s) - ts) * (vU + ad * dvU))
    return pL, pU


def quality(qb, c2, nan, ap, ad, counts3):
    """q of the last arrival of qf_value; counts3 = (n_d, n_p, nz)"""
    n_d, n_p, nz = (int(v) for v in counts3)
    ap, ad = F(ap), F(ad)
    if ap.view(np.int64) == 0 or ad.view(np.int64) == 0 or nan != 0.0:
        return INF
    with np.errstate(all="ignore"):
        ud, up = F(1.0) - ad, F(1.0) - ap
        td = ((ud * ud) * F(qb[D2])) / F(n_d) if n_d else F(0.0)
        tp = ((up * up) * F(qb[P2])) / F(n_p) if n_p else F(0.0)
        tc = F(c2) / F(nz)
        q = (td + tp) + tc
    return INF if np.isnan(q) else F(q)


def section_step(qb, q, c2, nan, ap, ad, qopts):
    """qf_section: ONE step of the state machine from the value q at the trial sigma — the own block after it"""
    b = qb.copy()
    ib = ints(b)
    tol, max_steps = F(qopts["section_sigma_tol"]), int(qopts["max_section_steps"])
    sigma = F(b[SIGMA])
    b[Q], b[C2], b[NANS], b[LAST_AP], b[LAST_AD] = q, c2, nan, ap, ad
    ib[EVALS] += 1
    if ib[EVALS] == 1 or q < b[QBEST]:
        b[BEST], b[QBEST] = sigma, q
    phase, steps = int(ib[PHASE]), int(ib[STEPS])
    lo_, hi_ = F(b[A_]), F(b[B_])
    done = step = False
    nxt = sigma
    g = F(GOLDEN)
    with np.errstate(all="ignore"):
        if phase == FIRST:
            b[Q0] = q
            nxt = np.maximum(F(b[LO]), sigma * (F(1.0) - F(1e-2)))
            phase = SECOND
        elif phase == SECOND:
            if q <= b[Q0]:
                lo_, hi_ = F(b[LO]), sigma
            else:
                lo_, hi_ = F(b[SIGMA0]), F(b[HI])
            w = hi_ - lo_
            if w <= tol * hi_:
                done = True
            else:
                gw = g * w
                b[C_], b[D_] = hi_ - gw, lo_ + gw
                nxt = F(b[C_])
                phase = LEFT
        elif phase == LEFT:
            b[QC] = q
            nxt = F(b[D_])
            phase = RIGHT
        elif phase == NEW_LEFT:
            b[QC] = q
            step = True
        else:
            b[QD] = q
            step = True
        if step:
            if steps >= max_steps:
                done = True
            else:
                if b[QC] <= b[QD]:
                    hi_ = F(b[D_])
                    b[D_], b[QD] = b[C_], b[QC]
                    gw = g * (hi_ - lo_)
                    b[C_] = hi_ - gw
                    nxt = F(b[C_])
                    phase = NEW_LEFT
                else:
                    lo_ = F(b[C_])
                    b[C_], b[QC] = b[D_], b[QD]
                    gw = g * (hi_ - lo_)
                    b[D_] = lo_ + gw
                    nxt = F(b[D_])
                    phase = NEW_RIGHT
                steps += 1
                if hi_ - lo_ <= tol * hi_:
                    done = True
    b[A_], b[B_] = lo_, hi_
    ib[PHASE], ib[STEPS] = phase, steps
    if done:
        ib[STATUS] = UNUSABLE if np.isposinf(b[QBEST]) else DONE
    else:
        b[SIGMA] = nxt
    b[ALPHA_P] = b[ALPHA_D] = 1.0
    return b


def value(B, st, d0, d1, qb, qopts, n_wg):
    """qf_value: the own block after the call; nothing unless a section is open"""
    if ints(qb)[STATUS] != SECTION:
        return qb.copy()
    ap, ad = F(qb[ALPHA_P]), F(qb[ALPHA_D])
    pL, pU = products(B, st, direction(d0, d1, scale(qb, qopts)), ap, ad)
    with np.errstate(all="ignore"):
        c2 = device_sum([pL * pL, pU * pU], n_wg)
        nan = device_sum([np.isnan(pL).astype(np.float64), np.isnan(pU).astype(np.float64)], n_wg)
    cn = B["counts"]
    q = quality(qb, c2, nan, ap, ad, (cn["nvar"] + cn["n_ineq"], cn["ncon"], cn["nz"]))
    return section_step(qb, q, c2, nan, ap, ad, qopts)


def section(B, st, d0, d1, qb, blk, qopts, n_wg, pairs=None, trace=None):
    """every alpha / value pair of a section (max_section_steps + 4): the own block after them; `trace` (a list) receives
    ``(sigma, q, block)`` per evaluation that ran"""
    pairs = int(qopts["max_section_steps"]) + 4 if pairs is None else pairs
    for _ in range(pairs):
        if ints(qb)[STATUS] != SECTION:
            break
        sigma = float(qb[SIGMA])
        qb = value(B, st, d0, d1, alpha(B, st, d0, d1, qb, blk, qopts), qopts, n_wg)
        if trace is not None:
            trace.append((sigma, float(qb[Q]), qb.copy()))
    return qb


def update(blk, ab, qb, w, counts, opts, aopts, force_fixed=False, ctl=None):
    """qf_update: ``(mu block, amu block, ctl)`` after the call — amu_reference.update word for word but for the free-mode oracle
    and the one more condition of UNUSABLE"""
    w = np.asarray(w, dtype=np.float64)
    blk, ab = blk.copy(), ab.copy()
    ctl = None if ctl is None else ctl.copy()
    nz = int(counts[1])
    e_d, e_p, sc = mref.terms(w, counts, opts)
    Emu = lambda mu: np.maximum(np.maximum(e_d, e_p), mref.e_c(w, counts, sc, mu))
    mu_old = F(blk[0])
    mu = mu_old
    floor, kappa_eps, kappa_mu = F(opts["mu_floor"]), F(opts["kappa_eps"]), F(opts["kappa_mu"])
    mu_min = F(aopts["mu_min"])
    e0, ec0 = Emu(F(0.0)), mref.e_c(w, counts, sc, F(0.0))
    k = 0
    unusable = w[10] != 0.0 or np.isnan(e0) or ints(qb)[STATUS] != DONE
    iw, ia = ints(blk), ints(ab)
    with np.errstate(all="ignore"):
        if unusable:
            status = mref.UNUSABLE
        elif e0 <= opts["tol"]:
            status = mref.CONVERGED
        elif nz == 0:
            status = mref.ITERATING
            mu = mu_min
        else:
            status = mref.ITERATING
            avg = w[9] / F(nz)
            ab[aref.AVG] = avg
            mu_hi = F(ab[aref.MU_MAX])
            if aref._is_plus_zero(mu_hi):
                mu_hi = F(aopts["mu_max_fact"]) * avg
                ab[aref.MU_MAX] = mu_hi
            nref = aref._ring(ab)
            progress = nref < aopts["refs_max"]
            if not progress:
                worst = F(ab[aref.REF0])
                for i in range(1, nref):
                    worst = np.maximum(worst, ab[aref.REF0 + i])
                progress = bool(e0 <= F(aopts["red_fact"]) * worst)
            mode = int(ia[aref.MODE])
            if mode == aref.FIXED:
                if progress:
                    mode = aref.FREE
                    ia[aref.TO_FREE] += 1
                    aref._remember(ab, aopts["refs_max"], e0)
                else:
                    while mu > floor and Emu(mu) <= kappa_eps * mu and k < mref.MAX_DECREASES:
                        mu = np.maximum(floor, np.minimum(kappa_mu * mu, mu * np.sqrt(mu)))
                        k += 1
            else:
                if progress and not force_fixed:
                    aref._remember(ab, aopts["refs_max"], e0)
                else:
                    mode = aref.FIXED
                    ia[aref.TO_FIXED] += 1
                    mu = np.minimum(np.maximum(F(aopts["init_factor"]) * avg, mu_min), mu_hi)
            ia[aref.MODE] = mode
            if mode == aref.FREE:
                sigma = F(qb[BEST])
                mu_or = sigma * avg
                ab[aref.MU_ORACLE], ab[aref.SIGMA], ab[aref.M_AFF] = mu_or, sigma, qb[QBEST]
                mu = np.minimum(np.maximum(mu_or, mu_min), mu_hi)
        mu = F(mu)
        if mu.view(np.int64) != mu_old.view(np.int64):
            blk[0], blk[1], blk[2] = mu, np.maximum(F(opts["tau_min"]), F(1.0) - mu), np.sqrt(mu)
            iw[9] |= 1
            if ctl is not None:
                ctl[11] = ctl[12] = 0.0
        else:
            iw[9] &= ~1
        iw[10] += k
        blk[3], blk[4], blk[5], blk[6], blk[7] = e0, Emu(mu), e_d, e_p, ec0
    iw[8] = status
    iw[11] += 1
    return blk, ab, ctl


def done_block(sigma, q=1.0):
    """an own block whose section is DONE with the result sigma"""
    b = fresh_block()
    ints(b)[STATUS] = DONE
    b[BEST], b[QBEST] = sigma, q
    return b


def two_columns(P, mu_ref=1.0, dw=1e-2, mus=()):
    """The two directions of one iteration at P's state on the host — barrier_reference.terms at mu = 0 and mu = mu_ref, scipy's LU
    of kkt_diag_reference.host_kkt_diag (delta_w = dw), barrier_reference.step at tau = 1 — as ``d0, d1`` = (sol, ds, dzL, dzU, dvL,
    dvU) with +0.0 on the equality rows of the slack side; and for every mu of `mus` the direction computed DIRECTLY at that mu"""
    import kkt_diag_reference as dref
    from scipy.sparse.linalg import splu
    B, st, om = P["B"], P["state"], P["om"]
    sigma, dcon, rhs0 = bref.terms(B, st, P["r"], P["c"], 0.0)
    lu = splu(dref.host_kkt_diag(om, st[0], st[2], sigma, dw, dcon + 0.0).tocsc())
    zero = tuple(np.zeros(om.ncon) for _ in range(3))

    def at(mu):
        rhs = bref.terms(B, st, P["r"], P["c"], mu)[2]
        sol = lu.solve(rhs)
        dirs, _ = bref.step(B, st, sol, zero, mu, 1.0)
        return (sol, *dirs)
    return at(0.0), at(mu_ref), [at(mu) for mu in mus]


def host_loop(om, tol=1e-8, max_iter=200, mu=0.1, qf_opts=None, log=None):
    """tests/qf_loop.py on the HOST alone, made of the restatements — barrier_reference (start, terms, step, update, merit),
    mu_reference.error_words (sums in numpy's order), `begin` / `section` / `update` above on a grid of one workgroup,
    search_reference (slope, begin, trial, accept) — around a dense solve of the regularised KKT system whose inertia the
    eigenvalues give (the delta_w retry of the loops).  What it shows: the restated rule converges before a GPU is asked.
    Returns dict(x, objective, iterations, error, status, failed, mus, modes, sigmas, to_fixed, to_free)."""
    import search_reference as sref
    from kkt_diag_reference import host_kkt_diag
    B = bref.relaxed_bounds(om.lvar, om.uvar, om.lcon, om.ucon, bref.RELAX)
    n, m = om.nvar, om.ncon
    counts = (B["counts"]["ncon"], B["counts"]["nz"])
    opts, aopts = mref.options(mu_init=mu, tol=tol), aref.options()
    qopts = options(aopts, **(qf_opts or {}))
    blk, ab = mref.fresh_block(opts), aref.fresh_block(aopts)
    zero = tuple(np.zeros(m) for _ in range(3))
    x = np.array(om.x0, dtype=np.float64)
    x, s, zL, zU, vL, vU = bref.start(B, x, om.cons(x), zero)
    y = np.zeros(m)
    ctl, filt = sref.block(status=sref.UNUSABLE), np.zeros((sref.OPTS["filter_capacity"], 2))
    out = dict(failed=0, mus=[], modes=[], sigmas=[], status=None)
    ine = ~B["eq"]
    for it in range(max_iter + 1):
        st = (x, s, y, zL, zU, vL, vU)
        c, g, f = om.cons(x), om.grad(x), om.obj(x)
        r = g + om.jtprod(x, y)
        head, sums, w8, w10, p = mref.error_words(B, st, r, c)
        w = np.array([*head, *(float(np.sum(t)) for t in sums), w8, float(np.sum(p)), w10, 0.0])
        sigma, dcon, rhs0 = bref.terms(B, st, r, c, 0.0)
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

        def at(mu_):
            sol = np.linalg.solve(state["K"], bref.terms(B, st, r, c, mu_)[2])
            dirs, alpha = bref.step(B, st, sol, zero, mu_, 1.0)
            return sol, dirs, alpha
        factorise()
        (s0, dr0, _), (s1, dr1, _) = at(0.0), at(qopts["mu_ref"])
        qb = begin(B, st, r, c, w, ab, aopts, qopts, 1)
        qb = section(B, st, (s0, *dr0), (s1, *dr1), qb, blk, qopts, 1)
        blk, ab, _ = update(blk, ab, qb, w, counts, opts, aopts)
        iw, ia = ints(blk), ints(ab)
        mu_k, tau, status = float(blk[0]), float(blk[1]), int(iw[8])
        if iw[9] & 1:
            sref.set_word(ctl, sref.COUNT, 0)
            sref.set_word(ctl, sref.FLAGS, 0)
        out.update(iterations=it, error=float(blk[3]), status=status, to_fixed=int(ia[aref.TO_FIXED]), to_free=int(ia[aref.TO_FREE]))
        out["mus"].append(mu_k); out["modes"].append(int(ia[aref.MODE])); out["sigmas"].append(float(qb[BEST]))
        if log:
            log(dict(iter=it, error=float(blk[3]), mu=mu_k, sigma=float(qb[BEST]), section=(int(ints(qb)[STATUS]), int(ints(qb)[EVALS])), mode=int(ia[aref.MODE]), f=f))
        if status != mref.ITERATING or it == max_iter:
            break
        rhs = bref.terms(B, st, r, c, mu_k)[2]
        accepted, factored = False, True
        for _ in range(8):
            if not factored:
                factorise()
            factored = False
            sol = np.linalg.solve(state["K"], rhs)
            dirs, alpha = bref.step(B, st, sol, zero, mu_k, tau)
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
