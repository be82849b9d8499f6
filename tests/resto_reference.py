"""numpy restatement of csrc/iem_resto_device.h — resto_enter, resto_enter_filter, resto_terms, resto_step, resto_merit, resto_begin,
resto_trial, resto_update, resto_error, resto_check, resto_leave, expression for expression (every operation on IEEE doubles, rounded
once, nothing contracted: what -ffp-contract=off makes of the kernels) — the test family `wachter_biegler`, the table of hand-built
return-test and filter-append cases the CPU and the GPU test share, and an interior-point loop on the host (dense solve, inertia from
eigenvalues) with the restoration phase.  TEST INFRASTRUCTURE: tests/test_resto.py (CPU) and tests/test_gpu_resto.py.

Bounds are the dictionary of barrier_reference.relaxed_bounds, the state is barrier_reference's tuple (x, s, y, zL, zU, vL, vU), a
search's control block is search_reference's float64 array of 16 words.  The object is a dict `R`: its vectors p, n, zp, zn, dp, dn,
dzp, dzn, pt, nt, sR, ws (ncon), xR, wx (nvar) and `blk`, a float64 array of 8 words (word 0 is int64).  Every function returns new
arrays; entries the kernels do not write (the slack side on equality rows, everything under a gate) keep what they held."""
import math

import numpy as np

import barrier_reference as bref
import search_reference as sref

NONE, ACTIVE, RETURN = 0, 1, 2
R_STATE, R_THETA_START, R_THETA, R_PHI, R_ZMAX = range(5)
ROWS = ("p", "n", "zp", "zn", "dp", "dn", "dzp", "dzn", "pt", "nt", "sR", "ws")      # the order of the object's one allocation
VARS = ("xR", "wx")
OPTS = dict(rho=1000.0, kappa_resto=0.9, bound_mult_reset_threshold=1000.0)
NAN = float("nan")


def new_object(nvar, ncon):
    """what iem_resto_create leaves: everything zero, state NONE"""
    R = {k: np.zeros(ncon) for k in ROWS}
    R.update({k: np.zeros(nvar) for k in VARS})
    R["blk"] = np.zeros(8)
    return R


def _copy(R, **kw):
    out = {k: v.copy() for k, v in R.items()}
    out.update(kw)
    return out


def weight(v):
    with np.errstate(all="ignore"):
        m = np.minimum(1.0, 1.0 / np.abs(v))
        return m * m


def infeasibility(B, c, s):
    with np.errstate(all="ignore"):
        return np.where(B["eq"], c - B["ceq"], c - s)


def enter(B, R, st, c, mu, opts=OPTS):
    """resto_enter: ``(R, state)``; the block is resto_enter_filter's"""
    x, s, y, zL, zU, vL, vU = st
    rho = opts["rho"]
    ine = ~B["eq"]
    with np.errstate(all="ignore"):
        inf = infeasibility(B, c, s)
        rho2 = 2.0 * rho
        h = (mu - rho * inf) / rho2
        n = h + np.sqrt(h * h + (mu * inf) / rho2)
        p = inf + n
        R = _copy(R, xR=x.copy(), wx=weight(x), sR=np.where(ine, s, R["sR"]), ws=np.where(ine, weight(s), R["ws"]), n=n, p=p, zp=mu / p, zn=mu / n)
        clip = lambda z, on: np.where(on, np.minimum(rho, z), z)
        st = (x.copy(), s.copy(), np.zeros(len(y)), clip(zL, B["hasL"]), clip(zU, B["hasU"]), clip(vL, B["gL"]), clip(vU, B["gU"]))
    return R, st


def filter_append(ctl, filt, f_theta, f_phi, cap):
    """the rule of search_accept's h-type branch: dominated entries leave first, order kept, a full filter sets flag bit 1"""
    ctl, filt = ctl.copy(), filt.copy()
    count = min(max(sref.word(ctl, sref.COUNT), 0), cap)
    keep = ~((filt[:count, 0] >= f_theta) & (filt[:count, 1] >= f_phi))
    kept = int(keep.sum())
    filt[:kept] = filt[:count][keep]
    if kept < cap:
        filt[kept] = (f_theta, f_phi)
        sref.set_word(ctl, sref.COUNT, kept + 1)
    else:
        sref.set_word(ctl, sref.COUNT, kept)
        sref.set_word(ctl, sref.FLAGS, sref.word(ctl, sref.FLAGS) | 2)
    return ctl, filt


def enter_filter(blk, ctl_o, filt_o, sopts=sref.OPTS):
    """resto_enter_filter: ``(blk, ORIGINAL block, ORIGINAL filter)``"""
    theta0, phi0 = float(ctl_o[sref.THETA0]), float(ctl_o[sref.PHI0])
    ctl_o, filt_o = filter_append(ctl_o, filt_o, (1.0 - sopts["gamma_theta"]) * theta0, phi0 - sopts["gamma_phi"] * theta0, int(sopts["filter_capacity"]))
    blk = blk.copy()
    blk[R_THETA_START] = theta0
    blk[R_THETA] = blk[R_PHI] = NAN
    blk.view(np.int64)[R_STATE] = ACTIVE
    return blk, ctl_o, filt_o


def _side(B, R, st, mu, zeta, opts):
    """barrier_reference._side and the restoration's per-entry quantities"""
    x, s, y = st[0], st[1], st[2]
    rho = opts["rho"]
    q = bref._side(B, st, mu)
    with np.errstate(all="ignore"):
        q["zw"] = zeta * R["wx"]
        q["zs"] = zeta * R["ws"]
        q["gx"] = (q["mu"] - q["ml"]) + q["zw"] * (x - R["xR"])
        q["gsr"] = (q["nu"] - q["nl"]) + q["zs"] * (s - R["sR"])
        q["sigs1"] = q["sigs"] + q["zs"]
        q["rs1"] = q["gsr"] - y
        q["Dp"], q["Dn"] = R["p"] / R["zp"], R["n"] / R["zn"]
        q["ep"] = (mu - R["p"] * (rho - y)) / R["zp"]
        q["en"] = (mu - R["n"] * (rho + y)) / R["zn"]
    return q


def terms(B, R, st, r, c, mu, zeta, opts=OPTS):
    """resto_terms: ``(sigma, dcon, rhs)``"""
    q = _side(B, R, st, mu, zeta, opts)
    with np.errstate(all="ignore"):
        sigma = (q["sl"] + q["su"]) + q["zw"]
        rhs_x = -(r + q["gx"])
        rc = (infeasibility(B, c, st[1]) - R["p"]) + R["n"]
        t = (rc - q["ep"]) + q["en"]
        D = q["Dp"] + q["Dn"]
        inv = 1.0 / q["sigs1"]
        dcon = np.where(B["eq"], D, inv + D)
        rhs_y = np.where(B["eq"], -t, -(t + q["rs1"] * inv))
    return sigma, dcon, np.concatenate([rhs_x, rhs_y])


def step(B, R, st, sol, bufs, mu, tau, zeta, opts=OPTS):
    """resto_step: ``((ds, dzL, dzU, dvL, dvU), alpha, R)``; bufs = (ds, dvL, dvU) as they were: entries on equality rows stay"""
    x, s, y, zL, zU, vL, vU = st
    rho = opts["rho"]
    nvar = len(x)
    dx, dy = sol[:nvar], sol[nvar:]
    q = _side(B, R, st, mu, zeta, opts)
    ine = ~B["eq"]
    every = np.ones(len(dy), dtype=bool)
    with np.errstate(all="ignore"):
        ds_all = (dy - q["rs1"]) / q["sigs1"]
        dzL = np.where(B["hasL"], (q["ml"] - zL) - q["sl"] * dx, 0.0)
        dzU = np.where(B["hasU"], (q["mu"] - zU) + q["su"] * dx, 0.0)
        dvL_all = np.where(B["gL"], (q["nl"] - vL) - q["tl"] * ds_all, 0.0)
        dvU_all = np.where(B["gU"], (q["nu"] - vU) + q["tu"] * ds_all, 0.0)
        dp = q["ep"] + q["Dp"] * dy
        dn = q["en"] - q["Dn"] * dy
        dzp = ((rho - y) - R["zp"]) - dy
        dzn = ((rho + y) - R["zn"]) + dy
        ap = bref._alpha([(((-tau) * q["dL"]) / dx, B["hasL"] & (dx < 0)), ((tau * q["dU"]) / dx, B["hasU"] & (dx > 0)),
                          (((-tau) * q["eL"]) / ds_all, B["gL"] & (ds_all < 0)), ((tau * q["eU"]) / ds_all, B["gU"] & (ds_all > 0)),
                          (((-tau) * R["p"]) / dp, every & (dp < 0)), (((-tau) * R["n"]) / dn, every & (dn < 0))])
        ad = bref._alpha([(((-tau) * zL) / dzL, B["hasL"] & (dzL < 0)), (((-tau) * zU) / dzU, B["hasU"] & (dzU < 0)),
                          (((-tau) * vL) / dvL_all, B["gL"] & (dvL_all < 0)), (((-tau) * vU) / dvU_all, B["gU"] & (dvU_all < 0)),
                          (((-tau) * R["zp"]) / dzp, every & (dzp < 0)), (((-tau) * R["zn"]) / dzn, every & (dzn < 0))])
        if np.isnan(sol).any() or np.isnan(ds_all[ine]).any() or np.isnan(dp).any() or np.isnan(dn).any():
            ap = 0.0
        if (np.isnan(dzL[B["hasL"]]).any() or np.isnan(dzU[B["hasU"]]).any() or np.isnan(dvL_all[B["gL"]]).any() or np.isnan(dvU_all[B["gU"]]).any() or
                np.isnan(dzp).any() or np.isnan(dzn).any()):
            ad = 0.0
    dirs = (np.where(ine, ds_all, bufs[0]), dzL, dzU, np.where(ine, dvL_all, bufs[1]), np.where(ine, dvU_all, bufs[2]))
    return dirs, np.array([ap, ad]), _copy(R, dp=dp, dn=dn, dzp=dzp, dzn=dzn)


def merit_terms(B, R, which, x, s, c):
    """the addends of resto_merit's four sums: ``(S0, S1, theta_R, L)`` at (x, s, c) with (p, n) or (pt, nt)"""
    p, n = (R["pt"], R["nt"]) if which else (R["p"], R["n"])
    ine = ~B["eq"]
    with np.errstate(all="ignore"):
        dxr, dsr = x - R["xR"], s - R["sR"]
        s1 = np.concatenate([R["wx"] * (dxr * dxr), (R["ws"] * (dsr * dsr))[ine]])
        rc = (infeasibility(B, c, s) - p) + n
        _, logs = bref.merit_terms(B, x, s, c)
        logs = np.concatenate([logs, np.log(p), np.log(n)])
    return p + n, s1, np.abs(rc), logs


def merit_out(S0, S1, theta, L, zeta, opts=OPTS):
    """what the last workgroup writes from the four totals"""
    return np.array([opts["rho"] * S0 + (0.5 * zeta) * S1, theta, L])


def merit(B, R, which, x, s, c, zeta, opts=OPTS):
    """resto_merit with numpy's sums (the host loop's; the device's sums are compared through merit_terms)"""
    return merit_out(*(float(t.sum()) for t in merit_terms(B, R, which, x, s, c)), zeta, opts)


def slope_terms(B, R, st, sol, ds, mu, zeta, opts=OPTS):
    """the addends of resto_begin's slope: gx·dx per variable, gsr·ds per inequality row, (rho − mu/p)·dp + (rho − mu/n)·dn per row"""
    q = _side(B, R, st, mu, zeta, opts)
    rho = opts["rho"]
    with np.errstate(all="ignore"):
        return np.concatenate([q["gx"] * sol[:len(st[0])], (q["gsr"] * ds)[~B["eq"]], (rho - mu / R["p"]) * R["dp"] + (rho - mu / R["n"]) * R["dn"]])


def merit_addends(B, R, which, x, s, c):
    """The four parked columns of resto_merit over [0, nvar + ncon) in the kernel's statement order: S0 (p + n, every row), S1 (the
    proximity term of a variable and of an inequality row), theta_R (every row), L (log gap lower then upper, then log p, log n on
    every row — numpy's logs)."""
    p, n = (R["pt"], R["nt"]) if which else (R["p"], R["n"])
    ine = ~B["eq"]
    every, allx = np.ones(len(c), dtype=bool), np.ones(len(x), dtype=bool)
    with np.errstate(all="ignore"):
        dxr, dsr = x - R["xR"], s - R["sR"]
        rc = (infeasibility(B, c, s) - p) + n
        logs = bref.log_addends(B, x, s) + [bref.full(B, None, None, every, np.log(p)), bref.full(B, None, None, every, np.log(n))]
        return ([bref.full(B, None, None, every, p + n)], [bref.full(B, allx, R["wx"] * (dxr * dxr), ine, R["ws"] * (dsr * dsr))],
                [bref.full(B, None, None, every, np.abs(rc))], logs)


def merit_device(B, R, which, x, s, c, zeta, n_wg, opts=OPTS):
    """resto_merit on a grid of `n_wg` workgroups: out[0] and out[1] carry the device's bits, out[2] is the device's order over
    numpy's logs"""
    return merit_out(*(bref.device_sum(col, n_wg) for col in merit_addends(B, R, which, x, s, c)), zeta, opts)


def slope_addends(B, R, st, sol, ds, mu, zeta, opts=OPTS):
    """the one parked column of resto_begin: gx·dx on a variable; on a row gsr·ds (inequality rows only), then
    (rho − mu/p)·dp + (rho − mu/n)·dn"""
    q = _side(B, R, st, mu, zeta, opts)
    rho = opts["rho"]
    nvar = len(st[0])
    every = np.ones(len(st[2]), dtype=bool)
    with np.errstate(all="ignore"):
        return [bref.full(B, np.ones(nvar, dtype=bool), q["gx"] * sol[:nvar], ~B["eq"], q["gsr"] * ds),
                bref.full(B, None, None, every, (rho - mu / R["p"]) * R["dp"] + (rho - mu / R["n"]) * R["dn"])]


def slope(B, R, st, sol, ds, mu, zeta, n_wg, opts=OPTS):
    """the slope resto_begin sums on a grid of `n_wg` workgroups: the device's bits"""
    return bref.device_sum(slope_addends(B, R, st, sol, ds, mu, zeta, opts), n_wg)


def error_addends(B, R, st, c):
    """The four parked columns of resto_error (out[4..7]): sum |y|, the multipliers (lower then upper, then zp, zn on every row),
    theta_R and L as resto_merit(0) adds them."""
    x, s, y, zL, zU, vL, vU = st
    every = np.ones(len(y), dtype=bool)
    _, _, theta, logs = merit_addends(B, R, 0, x, s, c)
    with np.errstate(all="ignore"):
        return ([bref.full(B, None, None, every, np.abs(y))],
                [bref.full(B, B["hasL"], zL, B["gL"], vL), bref.full(B, B["hasU"], zU, B["gU"], vU), bref.full(B, None, None, every, R["zp"]),
                 bref.full(B, None, None, every, R["zn"])], theta, logs)


def error_sums(B, R, st, c, n_wg):
    """out[4..7] of resto_error on a grid of `n_wg` workgroups (the last: the device's order over numpy's logs)"""
    return np.array([bref.device_sum(col, n_wg) for col in error_addends(B, R, st, c)])


def begin(ctl, slope, merit0, alpha, mu):
    """the INNER block resto_begin's last workgroup leaves, given the slope it summed: search_reference.begin word for word"""
    return sref.begin(ctl, slope, float(merit0[0]), np.array([0, 0, 0, 0, 0, 0, float(merit0[1]), float(merit0[2])]), alpha, mu, 1.0)


def trial(B, R, ctl, x, s, sol, ds, bufs):
    """resto_trial: ``(xt, st, R)``; everything stays under FAILED / UNUSABLE"""
    if sref.word(ctl, sref.STATUS) in (sref.FAILED, sref.UNUSABLE):
        return bufs[0].copy(), bufs[1].copy(), _copy(R)
    a = float(ctl[sref.ALPHA])
    xt, s_t = sref.trial(B, ctl, x, s, sol, ds, bufs)
    with np.errstate(all="ignore"):
        return xt, s_t, _copy(R, pt=R["p"] + a * R["dp"], nt=R["n"] + a * R["dn"])


def update(B, R, st, sol, dirs, alpha, mu, kappa=bref.KAPPA):
    """resto_update: ``(state, R)``; either step length +0.0: nothing moves"""
    ap, ad = float(alpha[0]), float(alpha[1])
    if not (ap > 0.0 and ad > 0.0):
        return tuple(a.copy() for a in st), _copy(R)
    new = bref.update(B, st, sol, dirs, alpha, mu, kappa)
    with np.errstate(all="ignore"):
        guard = lambda z, gap: np.minimum(np.maximum(z, mu / (kappa * gap)), (kappa * mu) / gap)
        p, n = R["p"] + ap * R["dp"], R["n"] + ap * R["dn"]
        return new, _copy(R, p=p, n=n, zp=guard(R["zp"] + ad * R["dzp"], p), zn=guard(R["zn"] + ad * R["dzn"], n))


def error(B, R, st, r, c, mu, zeta, opts=OPTS):
    """resto_error: ``(out[0..3] exactly, [terms of out[4]], ... [terms of out[7]])``; r = None: out[0] is NaN"""
    x, s, y, zL, zU, vL, vU = st
    rho = opts["rho"]
    ine = ~B["eq"]
    q = _side(B, R, st, mu, zeta, opts)
    with np.errstate(all="ignore"):
        t = (r if r is not None else np.zeros_like(x)) + q["zw"] * (x - R["xR"])
        t = np.where(B["hasL"], t - zL, t)
        t = np.where(B["hasU"], t + zU, t)
        u = q["zs"] * (s - R["sR"]) - y
        u = np.where(B["gL"], u - vL, u)
        u = np.where(B["gU"], u + vU, u)
        rc = (infeasibility(B, c, s) - R["p"]) + R["n"]
        dual = np.concatenate([u[ine], (rho - y) - R["zp"], (rho + y) - R["zn"]])
        comp = np.concatenate([(q["dL"] * zL - mu)[B["hasL"]], (q["dU"] * zU - mu)[B["hasU"]], (q["eL"] * vL - mu)[B["gL"]], (q["eU"] * vU - mu)[B["gU"]],
                               R["p"] * R["zp"] - mu, R["n"] * R["zn"] - mu])
    head = np.array([bref._max_abs(t) if r is not None else NAN, bref._max_abs(dual), bref._max_abs(rc), bref._max_abs(comp)])
    mult = np.concatenate([zL[B["hasL"]], zU[B["hasU"]], vL[B["gL"]], vU[B["gU"]], R["zp"], R["zn"]])
    _, _, theta, logs = merit_terms(B, R, 0, x, s, c)
    return head, np.abs(y), mult, theta, logs


def check(blk, ctl_o, filt_o, f, merit2, mu, opts=OPTS, cap=64):
    """resto_check: the object's block; anything but ACTIVE: as it was"""
    blk = blk.copy()
    if int(blk.view(np.int64)[R_STATE]) != ACTIVE:
        return blk
    theta = float(merit2[0])
    phi = float(f) - mu * float(merit2[1])
    count = min(max(sref.word(ctl_o, sref.COUNT), 0), cap)
    dominated = bool(((theta >= filt_o[:count, 0]) & (phi >= filt_o[:count, 1])).any())
    ok = (math.isfinite(theta) and math.isfinite(phi) and theta <= opts["kappa_resto"] * float(blk[R_THETA_START]) and theta <= float(ctl_o[sref.THETA_MAX])
          and not dominated)
    blk[R_THETA], blk[R_PHI] = theta, phi
    if ok:
        blk.view(np.int64)[R_STATE] = RETURN
    return blk


def leave(B, blk, st, opts=OPTS):
    """resto_leave: ``(state, blk)``: y = 0, the present bound multipliers 1.0 iff their maximum exceeds the threshold, state NONE"""
    x, s, y, zL, zU, vL, vU = st
    pairs = ((zL, B["hasL"]), (zU, B["hasU"]), (vL, B["gL"]), (vU, B["gU"]))
    with np.errstate(invalid="ignore"):
        zmax = max([bref._max_abs(z, on) for z, on in pairs])
    blk = blk.copy()
    blk[R_ZMAX] = zmax
    blk.view(np.int64)[R_STATE] = NONE
    if zmax > opts["bound_mult_reset_threshold"] or zmax != zmax:
        zL, zU, vL, vU = (np.where(on, 1.0, z) for z, on in pairs)
    return (x.copy(), s.copy(), np.zeros(len(y)), zL.copy(), zU.copy(), vL.copy(), vU.copy()), blk


# ---- the unreduced Newton system of the restoration barrier problem -------------------------------------------------------------------
def newton_blocks(P, R, K_parts, sol, dirs, dw, dc, mu, zeta, opts=OPTS):
    """barrier_reference.newton_blocks for the restoration problem at P's state and R, as residual vectors: stationarity in x, in s,
    in p, in n, the linearised constraints  J·dx − ds − dp + dn, and the linearised complementarity rows (bounds, then p·zp, n·zn).
    K_parts = (W, J) with W the Hessian of y'c (obj_weight = 0); r = J'y."""
    W, J = K_parts
    B = P["B"]
    x, s, y, zL, zU, vL, vU = P["state"]
    ds, dzL, dzU, dvL, dvU = dirs
    rho = opts["rho"]
    nvar = len(x)
    dx, dy = sol[:nvar], sol[nvar:]
    ine = ~B["eq"]
    z = lambda a, on: np.where(on, a, 0.0)
    zw, zs = zeta * R["wx"], zeta * R["ws"]
    r = J.T @ y
    with np.errstate(all="ignore"):
        b1 = (W @ dx + (zw + dw) * dx + J.T @ dy - z(dzL, B["hasL"]) + z(dzU, B["hasU"])) + (r + zw * (x - R["xR"]) - z(zL, B["hasL"]) + z(zU, B["hasU"]))
        b2 = z((zs * z(ds, ine) - dy - z(dvL, B["gL"]) + z(dvU, B["gU"])) + (zs * (s - R["sR"]) - y - z(vL, B["gL"]) + z(vU, B["gU"])), ine)
        bp = (-dy - R["dzp"]) + ((rho - y) - R["zp"])
        bn = (dy - R["dzn"]) + ((rho + y) - R["zn"])
        b3 = (J @ dx - z(ds, ine) - R["dp"] + R["dn"] - dc * dy) + ((infeasibility(B, P["c"], s) - R["p"]) + R["n"])
        b4 = np.concatenate([(zL * dx + (x - B["xl"]) * dzL - (mu - (x - B["xl"]) * zL))[B["hasL"]], (-zU * dx + (B["xu"] - x) * dzU - (mu - (B["xu"] - x) * zU))[B["hasU"]],
                             (vL * ds + (s - B["rl"]) * dvL - (mu - (s - B["rl"]) * vL))[B["gL"]], (-vU * ds + (B["ru"] - s) * dvU - (mu - (B["ru"] - s) * vU))[B["gU"]],
                             R["zp"] * R["dp"] + R["p"] * R["dzp"] - (mu - R["p"] * R["zp"]), R["zn"] * R["dn"] + R["n"] * R["dzn"] - (mu - R["n"] * R["zn"])])
    return b1, b2, bp, bn, b3, b4


# ---- the test family: Waechter and Biegler's counterexample, once per support ---------------------------------------------------------
def wachter_biegler(a, b, n=3, inequality=False, start=(-3.0, 1.0, 1.0)):
    """min ∫ x1 dt  s.t.  x1² − x2 + a == 0,  x1 − x3 − b == 0,  x2, x3 >= 0  pointwise over n supports of [0, 1] (Waechter and Biegler
    2000: a line-search interior-point method without a restoration phase gets stuck on it); `inequality`: x2, x3 become the slacks of
    the rows x1² + a >= 0, x1 − b >= 0.  The optimum is x1 = max(b, sqrt(−a)) wherever −a >= 0: the objective is that value."""
    from infiniteexamodels.jl_amd.infinite import InfiniteModel
    m = InfiniteModel()
    t = m.infinite_parameter("t", 0, 1, num_supports=n)
    x1 = m.variable("x[1]", t, start=start[0])
    m.objective("min", m.integral(x1, t))
    if inequality:
        m.constraint(x1 ** 2 + a >= 0.0)
        m.constraint(x1 - b >= 0.0)
    else:
        x2, x3 = m.variable("x[2]", t, lb=0.0, start=start[1]), m.variable("x[3]", t, lb=0.0, start=start[2])
        m.constraint(x1 ** 2 - x2 + a == 0.0)
        m.constraint(x1 - x3 - b == 0.0)
    return m


WB_MODELS = {"wb_eq": dict(a=1.0, b=1.0, inequality=False, optimum=1.0), "wb_ineq": dict(a=-1.0, b=2.0, inequality=True, optimum=2.0)}
_wb = {}


def wb_core(name, n=3):
    """the transcribed core of a named member of the family, built once per (name, n)"""
    if (name, n) not in _wb:
        from infiniteexamodels.jl_amd import transcribe
        kw = WB_MODELS[name]
        _wb[name, n] = transcribe.exa_core(wachter_biegler(kw["a"], kw["b"], n, kw["inequality"]))
    return _wb[name, n]


_points = {}


def wb_point(name, n=3, seed=0):
    """the shared state of a family member in the shape of barrier_reference.barrier_point: strictly interior, random multipliers"""
    if (name, n, seed) in _points:
        return _points[name, n, seed]
    from pyoracle import OracleModel
    core = wb_core(name, n)
    blob = core.to_blob()
    om = OracleModel(blob)
    B = bref.relaxed_bounds(om.lvar, om.uvar, om.lcon, om.ucon, bref.RELAX)
    rng = np.random.default_rng(2000 + seed)
    x = np.where(B["hasL"], B["xl"] + 10.0 ** rng.uniform(-2.0, 1.0, om.nvar), rng.uniform(-3.0, 3.0, om.nvar))
    y = rng.standard_normal(om.ncon)
    c = om.cons(x)
    with np.errstate(invalid="ignore"):
        s = np.where(B["eq"], NAN, np.where(B["gL"], B["rl"] + 10.0 ** rng.uniform(-2.0, 1.0, om.ncon), c))
    mult = lambda on: np.where(on, 10.0 ** rng.uniform(-2.0, 2.0, len(on)), NAN)
    st = (x, s, y, mult(B["hasL"]), mult(B["hasU"]), mult(B["gL"]), mult(B["gU"]))
    P = dict(core=core, blob=blob, om=om, B=B, lvar=om.lvar, uvar=om.uvar, lcon=om.lcon, ucon=om.ucon, state=st, r=om.grad(x) + om.jtprod(x, y), c=c, mu=bref.MU,
             tau=bref.TAU, relax=bref.RELAX)
    _points[name, n, seed] = P
    return P


def point(name, seed=0):
    """barrier_reference.barrier_point for the models of tests/cases.py, `wb_point` for "wb_eq", "wb_ineq" with "@n" for n supports"""
    if name.startswith("wb_"):
        base, _, n = name.partition("@")
        return wb_point(base, int(n or 3), seed)
    return bref.barrier_point(name, seed)


def entered(P, mu=None, seed=0, opts=OPTS):
    """An object in the middle of a phase at P's state, for the per-kernel tests: resto_enter at P (multipliers clipped, y drawn
    anew: enter zeroes it, a later iterate has one), then p, n, zp, zn moved off the central path by random factors and the reference
    point moved off the iterate.
    ``(R, state, mu)`` with mu = max(P["mu"], max |inf|) as the caller of enter forms it."""
    B = P["B"]
    rng = np.random.default_rng(3000 + seed)
    with np.errstate(invalid="ignore"):
        mu = max(P["mu"], float(np.abs(infeasibility(B, P["c"], P["state"][1])).max())) if mu is None else mu
    R, st = enter(B, new_object(len(P["state"][0]), len(P["c"])), P["state"], P["c"], mu, opts)
    m = len(P["c"])
    R = _copy(R, **{k: R[k] * 10.0 ** rng.uniform(-0.5, 0.5, m) for k in ("p", "n", "zp", "zn")})
    R["xR"] = R["xR"] + 0.05 * rng.standard_normal(len(R["xR"]))      # ... and the iterate has left the reference point
    R["sR"] = np.where(B["eq"], R["sR"], R["sR"] + 0.05 * rng.standard_normal(m))
    st = (st[0], st[1], P["state"][2].copy()) + st[3:]
    return R, st, mu


_big = {}
# barrier_reference.plant on the heavy lane of the sizes above 27 000 — weights and seeds (chosen so that tests/test_device_order.py
# passes): the direction (the slope), xR and sR (S1)
SPREAD_SOL, SPREAD_REF = (2.0 ** 30, 2.0 ** 31, 2.0 ** 50), (2.0 ** 10, 2.0 ** 10.5, 2.0 ** 11)
SEED_SOL, SEED_REF = 15, 0


def big_entered(supports):
    """`entered` at barrier_reference.big_point(supports) and one resto_step from a random sol, built once per size and left
    unchanged: dict(P, R (before the step), R_step (dp, dn, dzp, dzn filled), state, mu, zeta, sol, dirs, alpha).  On the heavy lane
    of the sizes above 27 000: the two variables get their heavy multipliers back (resto_enter clipped them to rho: the row keeps its
    clipped ones, a heavy row would leave no ds), and the direction and the reference point carry barrier_reference.plant's weights — so
    that the sum of the multipliers, the slope and S1 discriminate."""
    supports = int(supports)
    if supports not in _big:
        P = bref.big_point(supports)
        R, st, mu = entered(P)
        zeta = math.sqrt(mu)
        n, m = len(st[0]), len(st[2])
        sol = np.random.default_rng(4000 + supports // 10).standard_normal(n + m)
        if P["heavy"] is not None:
            iv = list(P["heavy"][:2])
            st = tuple(a.copy() for a in st)
            st[3][iv], st[4][iv] = P["state"][3][iv], P["state"][4][iv]
            R["xR"], R["sR"] = bref.plant(P, R["xR"], SPREAD_REF, SEED_REF), bref.plant(P, R["sR"], SPREAD_REF, SEED_REF)
            sol = bref.plant(P, sol, SPREAD_SOL, SEED_SOL)
        dirs, alpha, R_step = step(P["B"], R, st, sol, tuple(np.full(m, NAN) for _ in range(3)), mu, bref.TAU, zeta)
        _big[supports] = dict(P=P, R=R, R_step=R_step, state=st, mu=mu, zeta=zeta, sol=sol, dirs=dirs, alpha=alpha)
    return _big[supports]


# ---- the hand-built cases of the return test and of the filter append -----------------------------------------------------------------
def check_cases(cap=64):
    """``[(name, blk, ORIGINAL block, ORIGINAL filter, f, merit (2), mu, want state)]``: every branch of resto_check.  theta_start = 2,
    kappa_resto = 0.9: the ceiling is 1.8; mu = 0.1: phi = f − 0.1·merit[1]."""
    def blk(state=ACTIVE, theta_start=2.0):
        b = np.zeros(8)
        b.view(np.int64)[R_STATE] = state
        b[R_THETA_START] = theta_start
        b[R_THETA] = b[R_PHI] = NAN
        return b
    ob = dict(alpha=0.0, alpha_max=1.0, phi0=10.0, theta0=2.0, slope=-1.0, theta_min=1e-4, theta_max=1e4, status=sref.FAILED, trials=30, flags=1)
    far = lambda k, seed: sref._filter(sref._far(k, seed), cap)
    C = []
    add = lambda name, b, o, f, ft, m, want: C.append((name, b, sref.block(**o), f, ft, np.array(m, dtype=np.float64), 0.1, want))
    add("returns on an empty filter", blk(), ob, far(0, 1), 9.0, [1.0, 0.0], RETURN)
    add("returns with the log term in phi", blk(), dict(ob, count=1), sref._filter([(0.5, 8.95)], cap), 9.0, [1.0, 1.0], RETURN)
    add("dominated by a filter entry", blk(), dict(ob, count=3), sref._filter([(50.0, -1000.0), (0.5, 8.0), (55.0, -1001.0)], cap), 9.0, [1.0, 0.0], ACTIVE)
    add("theta above kappa_resto·theta_start", blk(), ob, far(0, 1), 9.0, [1.9, 0.0], ACTIVE)
    add("an equal theta at kappa_resto·theta_start returns", blk(), ob, far(0, 1), 9.0, [0.9 * 2.0, 0.0], RETURN)
    add("one ulp above kappa_resto·theta_start", blk(), ob, far(0, 1), 9.0, [float(np.nextafter(0.9 * 2.0, 2.0)), 0.0], ACTIVE)
    add("NaN theta", blk(), ob, far(0, 1), 9.0, [NAN, 0.0], ACTIVE)
    add("NaN f", blk(), ob, far(0, 1), NAN, [1.0, 0.0], ACTIVE)
    add("inf log term", blk(), ob, far(0, 1), 9.0, [1.0, float("-inf")], ACTIVE)
    add("theta above theta_max", blk(theta_start=1e6), dict(ob, theta_max=1e4), far(0, 1), 9.0, [2e4, 0.0], ACTIVE)
    add("theta equal to theta_max returns", blk(theta_start=1e6), dict(ob, theta_max=1e4), far(0, 1), 9.0, [1e4, 0.0], RETURN)
    add("63 entries, none dominates", blk(), dict(ob, count=63), far(63, 5), 9.0, [1.0, 0.0], RETURN)
    f64 = sref._far(64, 6)
    add("64 entries, none dominates", blk(), dict(ob, count=64), sref._filter(f64, cap), 9.0, [1.0, 0.0], RETURN)
    f64[-1] = (0.5, 8.0)
    add("64 entries, dominated by the last", blk(), dict(ob, count=64), sref._filter(f64, cap), 9.0, [1.0, 0.0], ACTIVE)
    add("state NONE: nothing is written", blk(state=NONE), ob, far(0, 1), 9.0, [1.0, 0.0], NONE)
    add("state RETURN: nothing is written", blk(state=RETURN), ob, far(0, 1), 9.0, [1.9, 0.0], RETURN)
    return C


def append_cases(cap=64):
    """``[(name, ORIGINAL block, ORIGINAL filter, want count, want overflow)]``: resto_enter_filter on filters of 0, 63, 64 (overflow)
    entries and with dominated entries that leave.  The new entry is (2·(1 − 1e-5), 10 − 2e-8)."""
    ob = dict(alpha=0.0, alpha_max=1.0, phi0=10.0, theta0=2.0, slope=-1.0, theta_min=1e-4, theta_max=1e4, phi_t=10.5, theta_t=2.5, status=sref.FAILED, trials=30, flags=1)
    C = [("empty filter", sref.block(**ob), sref._filter([], cap), 1, False),
         ("63 entries", sref.block(**dict(ob, count=63)), sref._filter(sref._far(63, 7), cap), 64, False),
         ("64 entries: overflow", sref.block(**dict(ob, count=64)), sref._filter(sref._far(64, 8), cap), 64, True)]
    mixed = [(50.0, -1000.0), (3.0, 11.0), (51.0, -1001.0), (2.5, 10.5), (1e3, 1e3), (52.0, -1002.0)]
    C.append(("dominated entries leave, order kept", sref.block(**dict(ob, count=6)), sref._filter(mixed, cap), 4, False))
    ent = [(3.0 + k, 11.0 + k) if k % 3 == 1 else e for k, e in enumerate(sref._far(64, 9))]
    C.append(("64 entries of which every third leaves", sref.block(**dict(ob, count=64)), sref._filter(ent, cap), 64 - 21 + 1, False))
    return C


# ---- an interior-point loop on the host with the restoration phase --------------------------------------------------------------------
KAPPA_EPS, KAPPA_MU, THETA_MU, TAU_MIN, DELTA_C = 10.0, 0.2, 1.5, 0.99, 1e-10


def _opt_err(head, sums, counts):
    m, nz = counts
    sd = max(100.0, (sums[0] + sums[1]) / max(1, m + nz)) / 100.0
    sc = max(100.0, sums[1] / max(1, nz)) / 100.0
    return max(max(head[0], head[1]) / sd, head[2], head[3] / sc if nz else 0.0)


def _solve_K(W, J, sigma, dcon, dw, rhs, m):
    """the delta_w retry of tests/search_loop.py on a dense matrix, inertia from eigenvalues"""
    tries = 0
    while True:
        K = np.block([[W + np.diag(sigma + dw), J.T], [J, -np.diag(dcon + DELTA_C)]])
        ev = np.linalg.eigvalsh(K)
        tries += 1
        if (np.isfinite(ev).all() and int((ev < 0).sum()) == m) or tries >= 24:
            break
        dw = 1e-4 if dw == 0.0 else dw * (100.0 if tries <= 2 else 8.0)
    return np.linalg.solve(K, rhs), dw


def _matrices(om, x, y, w):
    W, J = bref.oracle_matrices(om, x, y, w)
    return W.toarray(), J.toarray()


def host_restoration(om, B, st, mu_orig, ctl_o, filt_o, opts=OPTS, sopts=sref.OPTS, max_iter=100, log=None):
    """One restoration phase made of the restatements above around a dense solve — what tests/resto_loop.py does with the device
    objects.  ``(state or None, iterations, ORIGINAL block, ORIGINAL filter, why)``: None when the inner search fails or the cap is
    reached."""
    n_, m = om.nvar, om.ncon
    ine = ~B["eq"]
    c = om.cons(st[0])
    with np.errstate(invalid="ignore"):
        mu = max(mu_orig, float(np.abs(infeasibility(B, c, st[1])).max()))
    R, st = enter(B, new_object(n_, m), st, c, mu, opts)
    R["blk"], ctl_o, filt_o = enter_filter(R["blk"], ctl_o, filt_o, sopts)
    ctl, filt = sref.block(status=sref.UNUSABLE), np.zeros((sopts["filter_capacity"], 2))
    counts = (m, B["counts"]["nz"] + 2 * m)
    nanc = np.full(m, NAN)
    for it in range(max_iter):
        x, s, y = st[0], st[1], st[2]
        zeta = math.sqrt(mu)
        c = om.cons(x)
        r = om.jtprod(x, y)
        while mu > 1e-11:
            head, ay, mult, _, _ = error(B, R, st, r, c, mu, zeta, opts)
            if _opt_err(head, (float(ay.sum()), float(mult.sum())), counts) > KAPPA_EPS * mu:
                break
            mu = max(1e-11, min(KAPPA_MU * mu, mu ** THETA_MU))
            zeta = math.sqrt(mu)
            ctl, filt = sref.block(status=sref.UNUSABLE), np.zeros((sopts["filter_capacity"], 2))      # iem_search_reset(inner)
        tau = max(TAU_MIN, 1.0 - mu)
        sigma, dcon, rhs = terms(B, R, st, r, c, mu, zeta, opts)
        W, J = _matrices(om, x, y, 0.0)
        sol, dw = _solve_K(W, J, sigma, dcon, 0.0, rhs, m)
        dirs, alpha, R = step(B, R, st, sol, (nanc, nanc, nanc), mu, tau, zeta, opts)
        m0 = merit(B, R, 0, x, s, c, zeta, opts)
        ctl = begin(ctl, float(slope_terms(B, R, st, sol, dirs[0], mu, zeta, opts).sum()), m0, alpha, mu)
        d_alpha = alpha.copy()
        while sref.word(ctl, sref.STATUS) == sref.SEARCHING:
            xt, s_t, R = trial(B, R, ctl, x, s, sol, dirs[0], (x, s))
            mt = merit(B, R, 1, xt, s_t, om.cons(xt), zeta, opts)
            ctl, filt, d_alpha[0] = sref.accept(ctl, filt, mt[0], mt[1:], mu, 1.0, sopts)
        if sref.word(ctl, sref.STATUS) not in (sref.F_TYPE, sref.H_TYPE):
            return None, it + 1, ctl_o, filt_o, "inner search failed"
        st, R = update(B, R, st, sol, dirs, d_alpha, mu)
        c = om.cons(st[0])
        theta, logs = bref.merit_terms(B, st[0], st[1], c)
        R["blk"] = check(R["blk"], ctl_o, filt_o, om.obj(st[0]), np.array([float(theta.sum()), float(logs.sum())]), mu_orig, opts, sopts["filter_capacity"])
        if log:
            log(dict(resto_iter=it, mu=mu, alpha=float(d_alpha[0]), theta_R=float(ctl[sref.THETA_T]), theta=float(R["blk"][R_THETA]), dw=dw))
        if int(R["blk"].view(np.int64)[R_STATE]) == RETURN:
            st, _ = leave(B, R["blk"], st, opts)
            return st, it + 1, ctl_o, filt_o, "returned"
    return None, max_iter, ctl_o, filt_o, "no return within the cap"


def host_loop(om, x0=None, max_restorations=5, tol=1e-8, max_iter=200, mu=0.1, opts=OPTS, sopts=sref.OPTS, log=None):
    """tests/search_loop.py's loop made of the restatements, with bounds, around a dense solve; a FAILED search enters the restoration
    phase (`max_restorations = 0`: it ends the loop).  Returns dict(status = "solved" | "max_iter" | "search failed" | "restoration
    failed", x, objective, iterations, error, restorations, resto_iterations, why)."""
    B = bref.relaxed_bounds(om.lvar, om.uvar, om.lcon, om.ucon, bref.RELAX)
    n_, m = om.nvar, om.ncon
    nanc = np.full(m, NAN)
    x = np.array(om.x0 if x0 is None else x0, dtype=np.float64)
    x, s, zL, zU, vL, vU = bref.start(B, x, om.cons(x), (nanc, nanc, nanc))
    st = (x, s, np.zeros(m), zL, zU, vL, vU)
    ctl, filt = sref.block(status=sref.UNUSABLE), np.zeros((sopts["filter_capacity"], 2))
    counts = (m, B["counts"]["nz"])
    mu_floor = max(1e-11, tol / 10.0)
    out = dict(restorations=0, resto_iterations=0, why=None)
    for it in range(max_iter + 1):
        x, s, y = st[0], st[1], st[2]
        c, g = om.cons(x), om.grad(x)
        r = g + om.jtprod(x, y)
        head, ay, mult, theta, logs = bref.error(B, st, r, c, 0.0)
        err = _opt_err(head, (float(ay.sum()), float(mult.sum())), counts)
        out.update(iterations=it, error=err, x=x, objective=float(om.obj(x)))
        if err <= tol or it == max_iter:
            out["status"] = "solved" if err <= tol else "max_iter"
            return out
        changed = False
        while mu > mu_floor:
            head, ay, mult, _, _ = bref.error(B, st, r, c, mu)
            if _opt_err(head, (float(ay.sum()), float(mult.sum())), counts) > KAPPA_EPS * mu:
                break
            mu, changed = max(mu_floor, min(KAPPA_MU * mu, mu ** THETA_MU)), True
        if changed:
            ctl, filt = sref.block(status=sref.UNUSABLE), np.zeros((sopts["filter_capacity"], 2))
        tau = max(TAU_MIN, 1.0 - mu)
        sigma, dcon, rhs = bref.terms(B, st, r, c, mu)
        W, J = _matrices(om, x, y, 1.0)
        dw, ok = 0.0, False
        for _ in range(8):
            sol, dw = _solve_K(W, J, sigma, dcon, dw, rhs, m)
            dirs, alpha = bref.step(B, st, sol, (nanc, nanc, nanc), mu, tau)
            slope = float(sref.slope_terms(B, x, s, g, sol, dirs[0], mu).sum())
            ctl = sref.begin(ctl, slope, om.obj(x), np.array([0, 0, 0, 0, 0, 0, float(theta.sum()), float(logs.sum())]), alpha, mu)
            d_alpha = alpha.copy()
            while sref.word(ctl, sref.STATUS) == sref.SEARCHING:
                xt, s_t = sref.trial(B, ctl, x, s, sol, dirs[0], (x, s))
                th_t, lg_t = bref.merit_terms(B, xt, s_t, om.cons(xt))
                ctl, filt, d_alpha[0] = sref.accept(ctl, filt, om.obj(xt), np.array([float(th_t.sum()), float(lg_t.sum())]), mu, 1.0, sopts)
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
            out["status"] = "search failed"
            return out
        new, k, ctl, filt, why = host_restoration(om, B, st, mu, ctl, filt, opts, sopts, log=log)
        out["resto_iterations"] += k
        out["why"] = why
        if new is None:
            out["status"] = "restoration failed"
            return out
        out["restorations"] += 1
        st = new
    return out
