"""numpy restatement of csrc/iem_soc_device.h — soc_open, soc_rhs, soc_trial, soc_accept, soc_select, expression for expression
(every operation on IEEE doubles, rounded once, nothing contracted: what -ffp-contract=off makes of the kernels) — the test model
`maratos`, the table of hand-built correction cases the CPU and the GPU test share, and a Newton / filter loop on the host for
equality-constrained models without bounds.  TEST INFRASTRUCTURE: tests/test_soc.py (CPU) and tests/test_gpu_soc.py.

The acceptance test is NOT restated here: `accept` hands search_reference.accept a block whose alpha is alpha_max and whose search
cannot fail, and reads the decision, the filter and the two merit words off what comes back.  Bounds are the dictionary of
barrier_reference.relaxed_bounds; the control block is search_reference's float64 array of 16 words (13, 14 are int64)."""
import numpy as np

import barrier_reference as bref
import search_reference as sref

NONE, ACTIVE, ACCEPTED, CLOSED = 0, 1, 2, 3
SOC_STATE, SOC_ROUNDS, SOC_ALPHA_PREV = 13, 14, 15
OPTS = dict(max_soc=4, kappa_soc=0.99)
NAN = float("nan")


def open_(ctl):
    """soc_open: NONE becomes ACTIVE or CLOSED, any other state stays"""
    ctl = ctl.copy()
    if sref.word(ctl, SOC_STATE) != NONE:
        return ctl
    theta_t, theta0 = float(ctl[sref.THETA_T]), float(ctl[sref.THETA0])
    active = sref.word(ctl, sref.STATUS) == sref.SEARCHING and sref.word(ctl, sref.TRIALS) == 1 and bool(np.isfinite(theta_t)) and theta_t >= theta0
    if active:
        sref.set_word(ctl, SOC_ROUNDS, 0)
        ctl[SOC_ALPHA_PREV] = ctl[sref.ALPHA_MAX]
    sref.set_word(ctl, SOC_STATE, ACTIVE if active else CLOSED)
    return ctl


def rhs(B, ctl, st, c, ct, s_t, rhs1, csoc, buf, mu=bref.MU):
    """soc_rhs: ``(rhs_soc, csoc)``; `buf` = rhs_soc as it was, `csoc` the object's residual as it was: both stay unless ACTIVE"""
    if sref.word(ctl, SOC_STATE) != ACTIVE:
        return buf.copy(), csoc.copy()
    nvar = len(st[0])
    a_prev = float(ctl[SOC_ALPHA_PREV])
    q = bref._side(B, st, mu)
    with np.errstate(all="ignore"):
        prev = np.where(B["eq"], c - B["ceq"], c - st[1]) if sref.word(ctl, SOC_ROUNDS) == 0 else csoc
        new = a_prev * prev + np.where(B["eq"], ct - B["ceq"], ct - s_t)
        inv = 1.0 / q["sigs"]
        rhs_y = np.where(B["eq"], -new, -(new + q["rs"] * inv))
    return np.concatenate([rhs1[:nvar], rhs_y]), new


def trial(B, ctl, x, s, sol_soc, ds_soc, alpha_soc, bufs):
    """soc_trial: ``(xt, st)``; bufs = (xt, st) as they were: everything stays unless ACTIVE with alpha_soc[0] > 0"""
    a = float(alpha_soc[0])
    if sref.word(ctl, SOC_STATE) != ACTIVE or not a > 0.0:
        return bufs[0].copy(), bufs[1].copy()
    with np.errstate(all="ignore"):
        return x + a * sol_soc[:len(x)], np.where(~B["eq"], s + a * ds_soc, bufs[1])


def accept(ctl, filt, ft, merit, alpha_soc, d_alpha, mu, sigma=1.0, opts=sref.OPTS, soc_opts=OPTS):
    """soc_accept: ``(control block, filter, d_alpha)``; `d_alpha` the two words as they were"""
    ctl, filt, d_alpha = ctl.copy(), filt.copy(), np.array(d_alpha, dtype=np.float64)
    if sref.word(ctl, SOC_STATE) != ACTIVE:
        return ctl, filt, d_alpha
    rounds = sref.word(ctl, SOC_ROUNDS)
    a_soc = float(alpha_soc[0])
    if not a_soc > 0.0:
        sref.set_word(ctl, SOC_ROUNDS, rounds + 1)
        sref.set_word(ctl, SOC_STATE, CLOSED)
        return ctl, filt, d_alpha
    theta_prev = float(ctl[sref.THETA_T])
    probe = ctl.copy()      # the shared test, at the full step's alpha, in a search that cannot fail
    probe[sref.ALPHA] = ctl[sref.ALPHA_MAX]
    sref.set_word(probe, sref.TRIALS, 0)
    got, got_filt, _ = sref.accept(probe, filt, ft, merit, mu, sigma, dict(opts, max_trials=2 ** 62, alpha_floor=0.0))
    ctl[sref.PHI_T], ctl[sref.THETA_T] = got[sref.PHI_T], got[sref.THETA_T]
    sref.set_word(ctl, SOC_ROUNDS, rounds + 1)
    status = sref.word(got, sref.STATUS)
    if status in (sref.F_TYPE, sref.H_TYPE):
        filt = got_filt
        for w in (sref.STATUS, sref.COUNT, sref.FLAGS):
            sref.set_word(ctl, w, sref.word(got, w))
        ctl[sref.ALPHA] = a_soc
        d_alpha[0], d_alpha[1] = a_soc, float(alpha_soc[1])
        sref.set_word(ctl, SOC_STATE, ACCEPTED)
        return ctl, filt, d_alpha
    theta_t = float(ctl[sref.THETA_T])
    if rounds + 1 < soc_opts["max_soc"] and bool(np.isfinite(theta_t)) and theta_t <= soc_opts["kappa_soc"] * theta_prev:
        ctl[SOC_ALPHA_PREV] = a_soc
    else:
        sref.set_word(ctl, SOC_STATE, CLOSED)
    return ctl, filt, d_alpha


def select(B, ctl, sol_soc, dirs_soc, sol, dirs):
    """soc_select: ``(sol, (ds, dzL, dzU, dvL, dvU))``; the first-order direction as it was unless ACCEPTED"""
    if sref.word(ctl, SOC_STATE) != ACCEPTED:
        return sol.copy(), tuple(d.copy() for d in dirs)
    ine = ~B["eq"]
    pick = lambda new, old, rows: np.where(ine, new, old) if rows else new.copy()
    return sol_soc.copy(), tuple(pick(n_, o_, k in (0, 3, 4)) for k, (n_, o_) in enumerate(zip(dirs_soc, dirs)))


# ---- the test model: the Maratos effect on a circle, once per support ---------------------------------------------------------------
def maratos(n=3):
    """x1(t), x2(t) over n supports, no bounds: min ∫ 2(x1² + x2² − 1) − x1 dt  s.t.  x1² + x2² == 1 pointwise (Nocedal and Wright,
    example 15.4, per support).  The optimum is x = (1, 0), y_k = −1.5·w_k with w_k the quadrature weights."""
    from infiniteexamodels.jl_amd.infinite import InfiniteModel
    m = InfiniteModel()
    t = m.infinite_parameter("t", 0, 1, num_supports=n)
    x = [m.variable(f"x[{i + 1}]", t) for i in range(2)]
    m.objective("min", m.integral(2 * (x[0] ** 2 + x[1] ** 2 - 1) - x[0], t))
    m.constraint(x[0] ** 2 + x[1] ** 2 == 1.0)
    return m


_maratos = {}


def maratos_point(angle=0.8, y_scale=-1.5, n=3):
    """The shared state of `maratos` in the shape of barrier_reference.barrier_point, built once and left unchanged: x = (cos angle,
    sin angle) at every support, y_k = y_scale·w_k; every row is an equality, so s, vL, vU are NaN and zL, zU are NaN (no bounds).
    The weights are read off grad f at x = 0 (−w_k on x1(t_k)), the pairing of x1, x2 and rows off the Jacobian's structure."""
    key = (angle, y_scale, n)
    if key in _maratos:
        return _maratos[key]
    from infiniteexamodels.jl_amd import transcribe
    from pyoracle import OracleModel
    core = transcribe.exa_core(maratos(n))
    blob = core.to_blob()
    om = OracleModel(blob)
    B = bref.relaxed_bounds(om.lvar, om.uvar, om.lcon, om.ucon, bref.RELAX)
    assert om.nvar == 2 * n and om.ncon == n and B["eq"].all() and B["counts"]["nz"] == 0
    g0 = om.grad(np.zeros(om.nvar))
    first = np.nonzero(g0)[0]
    jr, jc = om.jac_structure()
    x, y, w = np.zeros(om.nvar), np.zeros(om.ncon), np.zeros(om.ncon)
    for j in range(om.ncon):
        cols = jc[jr == j]
        i1 = next(int(i) for i in cols if i in first)
        i2 = next(int(i) for i in cols if i not in first)
        x[i1], x[i2], w[j] = np.cos(angle), np.sin(angle), -g0[i1]
        y[j] = y_scale * w[j]
    nanv, nanc = np.full(om.nvar, NAN), np.full(om.ncon, NAN)
    c = om.cons(x)
    P = dict(core=core, blob=blob, om=om, B=B, lvar=om.lvar, uvar=om.uvar, lcon=om.lcon, ucon=om.ucon, state=(x, nanc.copy(), y, nanv.copy(), nanv.copy(), nanc.copy(), nanc.copy()),
             r=om.grad(x) + om.jtprod(x, y), c=c, mu=bref.MU, tau=bref.TAU, relax=bref.RELAX, weights=w)
    _maratos[key] = P
    return P


def point(name, seed=0):
    """barrier_reference.barrier_point for the models of tests/cases.py, `maratos_point` for "maratos" """
    return maratos_point() if name == "maratos" else bref.barrier_point(name, seed)


# ---- a Newton / filter loop on the host, for equality-constrained models without bounds ---------------------------------------------
def host_loop(om, x0, y0, max_soc=4, tol=1e-8, max_iter=50, mu=0.1, opts=sref.OPTS, soc_opts=OPTS, log=None):
    """Algorithm A made of the restatements (search_reference.begin / accept, open_ / rhs / trial / accept above) around a dense
    solve of the exact Newton system — what tests/soc_loop.py does with the device objects, for a model whose rows are all equalities
    and whose variables are free (sigma = 0, no slack, alpha_max = 1, phi = f).  max_soc = 0 leaves the correction out.
    Returns dict(x, y, iterations, error, rejected, soc_accepted, soc_rounds, failed, first)."""
    from kkt_diag_reference import host_kkt_diag
    B = bref.relaxed_bounds(om.lvar, om.uvar, om.lcon, om.ucon, bref.RELAX)
    assert B["eq"].all() and B["counts"]["nz"] == 0
    n, m = om.nvar, om.ncon
    x, y = np.array(x0, dtype=np.float64), np.array(y0, dtype=np.float64)
    nanv, nanc = np.full(n, NAN), np.full(m, NAN)
    ctl, filt = sref.block(status=sref.UNUSABLE), np.zeros((opts["filter_capacity"], 2))
    so = dict(soc_opts, max_soc=max(1, max_soc))
    out = dict(rejected=0, soc_accepted=0, soc_rounds=0, failed=0, first=None)
    for it in range(max_iter + 1):
        st = (x, nanc, y, nanv, nanv, nanc, nanc)
        c, g = om.cons(x), om.grad(x)
        r = g + om.jtprod(x, y)
        err = max(float(np.abs(r).max()) / (max(100.0, float(np.abs(y).sum()) / m) / 100.0), float(np.abs(c - B["ceq"]).max()))
        out.update(iterations=it, error=err)
        if err <= tol or it == max_iter:
            break
        _, _, rhs1 = bref.terms(B, st, r, c, mu)
        K = host_kkt_diag(om, x, y, np.zeros(n), 0.0, 0.0).toarray()
        sol = np.linalg.solve(K, rhs1)
        alpha = np.array([1.0, 1.0])
        theta0 = float(np.abs(c - B["ceq"]).sum())
        ctl = sref.begin(ctl, float((g * sol[:n]).sum()), om.obj(x), np.array([0, 0, 0, 0, 0, 0, theta0, 0.0]), alpha, mu)
        d_alpha = alpha.copy()
        rung = 0
        while sref.word(ctl, sref.STATUS) == sref.SEARCHING:
            xt, _ = sref.trial(B, ctl, x, nanc, sol, nanc, (nanv, nanc))
            ct = om.cons(xt)
            merit = np.array([float(np.abs(ct - B["ceq"]).sum()), 0.0])
            ctl, filt, d_alpha[0] = sref.accept(ctl, filt, om.obj(xt), merit, mu, 1.0, opts)
            rung += 1
            if rung == 1 and max_soc > 0:
                ctl = open_(ctl)
                csoc = np.zeros(m)
                while sref.word(ctl, SOC_STATE) == ACTIVE:
                    rhs_soc, csoc = rhs(B, ctl, st, c, ct, nanc, rhs1, csoc, np.full(n + m, NAN), mu)
                    sol_soc = np.linalg.solve(K, rhs_soc)
                    xt, _ = trial(B, ctl, x, nanc, sol_soc, nanc, alpha, (nanv, nanc))
                    ct = om.cons(xt)
                    merit = np.array([float(np.abs(ct - B["ceq"]).sum()), 0.0])
                    ctl, filt, d_alpha = accept(ctl, filt, om.obj(xt), merit, alpha, d_alpha, mu, 1.0, opts, so)
                    out["soc_rounds"] += 1
                if sref.word(ctl, SOC_STATE) == ACCEPTED:
                    out["soc_accepted"] += 1
                    sol = sol_soc
                if out["first"] is None:
                    out["first"] = dict(state=sref.word(ctl, SOC_STATE), status=sref.word(ctl, sref.STATUS), rounds=sref.word(ctl, SOC_ROUNDS))
        out["rejected"] += sref.word(ctl, sref.TRIALS)
        if log:
            log(dict(iter=it, error=err, status=sref.word(ctl, sref.STATUS), trials=sref.word(ctl, sref.TRIALS), soc=sref.word(ctl, SOC_STATE), alpha=float(d_alpha[0])))
        if sref.word(ctl, sref.STATUS) not in (sref.F_TYPE, sref.H_TYPE):
            out["failed"] += 1
            break
        x, y = x + d_alpha[0] * sol[:n], y + d_alpha[0] * sol[n:]
    out.update(x=x, y=y)
    return out


# ---- the hand-built cases: one per branch of soc_open and soc_accept --------------------------------------------------------------
def cases(cap=64):
    """``[(name, control block behind the first rung, filter, rounds, opts, soc_opts, what)]`` with `rounds` a list of
    ``(alpha_soc (2), ft, merit (2))`` — what the barrier step, the objective and the merit sums hand soc_accept round by round — and
    `what` the expected ``dict(state, status, rounds[, count, overflow])`` after open and the rounds.  mu = 0.1, sigma = 1: phi_t =
    ft − 0.1·merit[1].  The grounds are those of search_reference.cases, one rejected trial in: alpha = alpha_max/2, trials = 1."""
    o = dict(sref.OPTS, filter_capacity=cap)
    so = dict(OPTS)
    # f-type ground (switching holds): the rejected first trial raised theta from 1e-6 to 0.5 and failed Armijo
    fb = dict(alpha=0.5, alpha_max=1.0, phi0=10.0, theta0=1e-6, slope=-2.0, theta_min=1e-4, theta_max=1e4, phi_t=10.5, theta_t=0.5, status=sref.SEARCHING, trials=1, flags=1)
    # h-type ground: theta0 = 2 > theta_min; the rejected first trial: theta 2.5, phi 10.5
    hb = dict(fb, theta0=2.0, theta_t=2.5)
    A = (0.75, 0.5)      # alpha_soc: not alpha_max, so that a mix-up of the two shows
    C = []

    def add(name, b, f, seq, opts=o, soc_opts=so, **what):
        C.append((name, sref.block(**b), sref._filter(f, opts["filter_capacity"]), [(np.array(a, dtype=np.float64), ft, np.array(m, dtype=np.float64)) for a, ft, m in seq],
                  opts, soc_opts, what))
    ok_f, ok_h, bad = (A, 9.0, [1e-7, 0.0]), (A, 9.0, [1.0, 0.0]), (A, 10.5, [2.4, 0.0])
    # open / not open
    add("not open: the first trial was accepted", dict(hb, status=sref.H_TYPE, trials=0, alpha=1.0), [], [ok_h], state=CLOSED, status=sref.H_TYPE, rounds=0)
    add("not open: the search failed (max_trials = 1)", dict(hb, status=sref.FAILED, alpha=0.0), [], [ok_h], state=CLOSED, status=sref.FAILED, rounds=0)
    add("not open: UNUSABLE", dict(hb, status=sref.UNUSABLE, alpha=0.0, trials=0), [], [ok_h], state=CLOSED, status=sref.UNUSABLE, rounds=0)
    add("not open: two trials rejected", dict(hb, trials=2, alpha=0.25), [], [ok_h], state=CLOSED, status=sref.SEARCHING, rounds=0)
    add("not open: no trial yet", dict(hb, trials=0, alpha=1.0, theta_t=NAN, phi_t=NAN), [], [ok_h], state=CLOSED, status=sref.SEARCHING, rounds=0)
    add("not open: theta_t < theta0", dict(hb, theta_t=1.999999), [], [ok_h], state=CLOSED, status=sref.SEARCHING, rounds=0)
    add("not open: theta_t NaN", dict(hb, theta_t=NAN), [], [ok_h], state=CLOSED, status=sref.SEARCHING, rounds=0)
    add("not open: theta_t inf", dict(hb, theta_t=float("inf")), [], [ok_h], state=CLOSED, status=sref.SEARCHING, rounds=0)
    add("open: theta_t == theta0", dict(hb, theta_t=2.0), [], [], state=ACTIVE, status=sref.SEARCHING, rounds=0)
    add("already ACCEPTED: nothing moves", dict(hb, status=sref.F_TYPE, alpha=0.75), [], [ok_h], state=ACCEPTED, status=sref.F_TYPE, rounds=1, preset=(ACCEPTED, 1, 1.0))
    add("already CLOSED: nothing moves", hb, [], [ok_h], state=CLOSED, status=sref.SEARCHING, rounds=2, preset=(CLOSED, 2, 0.75))
    # accepted
    add("accepted f-type in round 1", fb, [], [ok_f, ok_f], state=ACCEPTED, status=sref.F_TYPE, rounds=1)
    # 1e-3^2.3 = 1.26e-7 against 3.8e-7^1.1 = 8.7e-8: the switching condition holds with alpha_max = 1, not with word 0 = 0.5 nor with alpha_soc
    add("f-type needs alpha_max in the switching condition", dict(fb, slope=-1e-3, theta0=3.8e-7, theta_t=0.5), [], [((1e-9, 0.5), 9.0, [1e-9, 0.0])],
        state=ACCEPTED, status=sref.F_TYPE, rounds=1)
    add("accepted h-type by theta", hb, [], [ok_h], state=ACCEPTED, status=sref.H_TYPE, rounds=1, count=1)
    add("accepted h-type by phi in round 2", hb, [], [(A, 10.5, [2.4, 0.0]), ((0.625, 0.25), 9.0, [3.0, 0.0])], state=ACCEPTED, status=sref.H_TYPE, rounds=2, count=1)
    for k in sref.filter_sizes(cap):
        if k in (0, 63, 64, 65):
            far = sref._far(k, 3 + k)
            ent = [(3.0 + i, 11.0 + i) if i % 3 == 1 else far[i] for i in range(k)]      # every third entry is dominated by the new one
            add(f"accepted h-type on a filter of {k}", dict(hb, count=k), ent, [ok_h], state=ACCEPTED, status=sref.H_TYPE, rounds=1, count=k - len(range(1, k, 3)) + 1)
    add("accepted h-type on a full filter", dict(hb, count=cap), sref._far(cap, 2), [ok_h], state=ACCEPTED, status=sref.H_TYPE, rounds=1, count=cap, overflow=True)
    # rejected
    add("rejected, continuing (theta 2.5 -> 2.4 -> 2.3)", hb, [], [bad, ((0.625, 0.25), 10.5, [2.3, 0.0])], state=ACTIVE, status=sref.SEARCHING, rounds=2)
    add("rejected by kappa_soc (theta 2.5 -> 2.49)", hb, [], [(A, 10.5, [2.49, 0.0]), ok_h], state=CLOSED, status=sref.SEARCHING, rounds=1)
    add("rejected by kappa_soc in round 2 (theta 2.4 -> 2.39)", hb, [], [bad, (A, 10.5, [2.39, 0.0]), ok_h], state=CLOSED, status=sref.SEARCHING, rounds=2)
    add("rejected: dominated by a filter entry, continuing", dict(hb, count=1), [(0.5, 8.0)], [ok_h], state=ACTIVE, status=sref.SEARCHING, rounds=1)
    add("rejected: theta_t NaN closes", hb, [], [(A, 9.0, [NAN, 0.0]), ok_h], state=CLOSED, status=sref.SEARCHING, rounds=1)
    add("rejected: phi_t NaN, theta fine, continuing", hb, [], [(A, NAN, [1.0, 0.0])], state=ACTIVE, status=sref.SEARCHING, rounds=1)
    add("rejected at max_soc = 4", hb, [], [(A, 10.5, [2.4 - 0.1 * k, 0.0]) for k in range(4)] + [ok_h], state=CLOSED, status=sref.SEARCHING, rounds=4)
    add("rejected at max_soc = 1", hb, [], [bad, ok_h], soc_opts=dict(so, max_soc=1), state=CLOSED, status=sref.SEARCHING, rounds=1)
    add("kappa_soc = 1: an equal theta continues", dict(hb, theta_t=2.5), [], [(A, 10.5, [2.5, 0.0])], soc_opts=dict(so, kappa_soc=1.0), state=ACTIVE, status=sref.SEARCHING, rounds=1)
    # unusable alpha_soc
    add("unusable alpha_soc (+0.0)", hb, [], [((0.0, 0.5), 9.0, [1.0, 0.0]), ok_h], state=CLOSED, status=sref.SEARCHING, rounds=1)
    add("unusable alpha_soc (NaN) in round 2", hb, [], [bad, ((NAN, 0.5), 9.0, [1.0, 0.0]), ok_h], state=CLOSED, status=sref.SEARCHING, rounds=2)
    return C


def run_case(case, d_alpha=(0.0, 0.625)):
    """open and every round of a case through the restatement: the list of ``(block, filter, d_alpha)`` after open and after each round"""
    name, ctl, filt, rounds, o, so, what = case
    if "preset" in what:
        ctl = ctl.copy()
        sref.set_word(ctl, SOC_STATE, what["preset"][0]); sref.set_word(ctl, SOC_ROUNDS, what["preset"][1]); ctl[SOC_ALPHA_PREV] = what["preset"][2]
    ctl = open_(ctl)
    d = np.array(d_alpha, dtype=np.float64)
    out = [(ctl, filt, d)]
    for a, ft, m in rounds:
        ctl, filt, d = accept(ctl, filt, ft, m, a, d, 0.1, 1.0, o, so)
        out.append((ctl, filt, d))
    return out
