"""numpy restatement of csrc/iem_barrier_device.h — barrier_start, barrier_terms, barrier_step, barrier_update, barrier_error,
barrier_merit, expression for expression (numpy rounds every operation and contracts nothing: what -ffp-contract=off makes of the
kernels) — and the state the tests of the barrier layer share.  TEST INFRASTRUCTURE: tests/test_barrier.py (CPU) and
tests/test_gpu_barrier.py.

Vectors are full length: x, zL, zU (nvar); s, vL, vU, ds, dvL, dvU (ncon, entries on equality rows never read or written).  Where
the kernels branch on a presence flag the restatement computes on every entry and selects with np.where: the selected entries
carry the same bits, the others (NaN / inf arithmetic on absent bounds) are discarded."""
import math

import numpy as np

MU, TAU, RELAX, KAPPA = 0.1, 0.99, 1e-8, 1e10
PUSH, FRAC = 1e-2, 1e-2
NAN = float("nan")


def relaxed_bounds(lvar, uvar, lcon, ucon, relax=RELAX):
    """dict(xl, xu, rl, ru, ceq, hasL, hasU, gL, gU, eq, counts) as iem_barrier_create forms them on the host"""
    lvar, uvar, lcon, ucon = (np.asarray(a, dtype=np.float64) for a in (lvar, uvar, lcon, ucon))
    with np.errstate(invalid="ignore"):
        lo = lambda b: np.where(np.isfinite(b), b - relax * np.maximum(1.0, np.abs(b)), -np.inf)
        hi = lambda b: np.where(np.isfinite(b), b + relax * np.maximum(1.0, np.abs(b)), np.inf)
        eq = lcon == ucon
        B = dict(xl=lo(lvar), xu=hi(uvar), rl=np.where(eq, -np.inf, lo(lcon)), ru=np.where(eq, np.inf, hi(ucon)), ceq=np.where(eq, lcon, 0.0), eq=eq)
    B["hasL"], B["hasU"] = np.isfinite(lvar), np.isfinite(uvar)
    B["gL"], B["gU"] = ~eq & np.isfinite(lcon), ~eq & np.isfinite(ucon)
    B["counts"] = dict(nvar=len(lvar), ncon=len(lcon), n_eq=int(eq.sum()), n_ineq=int((~eq).sum()), n_xl=int(B["hasL"].sum()), n_xu=int(B["hasU"].sum()),
                       n_sl=int(B["gL"].sum()), n_su=int(B["gU"].sum()))
    B["counts"]["nz"] = sum(B["counts"][k] for k in ("n_xl", "n_xu", "n_sl", "n_su"))
    return B


def push(v, lo, hi, has_lo, has_hi, k1=PUSH, k2=FRAC):
    """bar_push: Ipopt's projection into the interior"""
    with np.errstate(invalid="ignore"):
        both = has_lo & has_hi
        pl = k1 * np.maximum(np.abs(lo), 1.0)
        pl = np.where(both, np.minimum(pl, k2 * (hi - lo)), pl)
        v = np.where(has_lo, np.maximum(v, lo + pl), v)
        pu = k1 * np.maximum(np.abs(hi), 1.0)
        pu = np.where(both, np.minimum(pu, k2 * (hi - lo)), pu)
        return np.where(has_hi, np.minimum(v, hi - pu), v)


def start(B, x, c, bufs, k1=PUSH, k2=FRAC):
    """``(x, s, zL, zU, vL, vU)``; bufs = (s, vL, vU) as they were: entries on equality rows stay"""
    ine = ~B["eq"]
    x = push(x, B["xl"], B["xu"], B["hasL"], B["hasU"], k1, k2)
    s = np.where(ine, push(c, B["rl"], B["ru"], B["gL"], B["gU"], k1, k2), bufs[0])
    return (x, s, np.where(B["hasL"], 1.0, 0.0), np.where(B["hasU"], 1.0, 0.0), np.where(ine, np.where(B["gL"], 1.0, 0.0), bufs[1]),
            np.where(ine, np.where(B["gU"], 1.0, 0.0), bufs[2]))


def _side(B, st, mu):
    """the shared per-entry quantities: gaps, z/gap and mu/gap with exact +0.0 where a bound is absent"""
    x, s, y, zL, zU, vL, vU = st
    with np.errstate(all="ignore"):
        dL, dU, eL, eU = x - B["xl"], B["xu"] - x, s - B["rl"], B["ru"] - s
        q = dict(dL=dL, dU=dU, eL=eL, eU=eU)
        q["sl"], q["su"] = np.where(B["hasL"], zL / dL, 0.0), np.where(B["hasU"], zU / dU, 0.0)
        q["ml"], q["mu"] = np.where(B["hasL"], mu / dL, 0.0), np.where(B["hasU"], mu / dU, 0.0)
        q["tl"], q["tu"] = np.where(B["gL"], vL / eL, 0.0), np.where(B["gU"], vU / eU, 0.0)
        q["nl"], q["nu"] = np.where(B["gL"], mu / eL, 0.0), np.where(B["gU"], mu / eU, 0.0)
        q["sigs"] = q["tl"] + q["tu"]
        q["rs"] = (q["nu"] - q["nl"]) - y
    return q


def terms(B, st, r, c, mu=MU):
    """``(sigma, dcon, rhs)``"""
    q = _side(B, st, mu)
    with np.errstate(all="ignore"):
        sigma = q["sl"] + q["su"]
        rhs_x = -(r + (q["mu"] - q["ml"]))
        inv = 1.0 / q["sigs"]
        dcon = np.where(B["eq"], 0.0, inv)
        rhs_y = np.where(B["eq"], -(c - B["ceq"]), -((c - st[1]) + q["rs"] * inv))
    return sigma, dcon, np.concatenate([rhs_x, rhs_y])


def _alpha(cands):
    best = 1.0
    for cand, on in cands:
        if on.any():
            v = cand[on]
            with np.errstate(invalid="ignore"):
                v = np.where(v > 0.0, v, 0.0)      # not > 0 (a NaN, on or outside a bound): +0.0
            best = min(best, float(v.min()))
    return best


def step(B, st, sol, bufs, mu=MU, tau=TAU):
    """``((ds, dzL, dzU, dvL, dvU), alpha)``; bufs = (ds, dvL, dvU) as they were: entries on equality rows stay"""
    x, s, y, zL, zU, vL, vU = st
    nvar = len(x)
    dx, dy = sol[:nvar], sol[nvar:]
    q = _side(B, st, mu)
    ine = ~B["eq"]
    with np.errstate(all="ignore"):
        ds_all = (dy - q["rs"]) / q["sigs"]
        dzL = np.where(B["hasL"], (q["ml"] - zL) - q["sl"] * dx, 0.0)
        dzU = np.where(B["hasU"], (q["mu"] - zU) + q["su"] * dx, 0.0)
        dvL_all = np.where(B["gL"], (q["nl"] - vL) - q["tl"] * ds_all, 0.0)
        dvU_all = np.where(B["gU"], (q["nu"] - vU) + q["tu"] * ds_all, 0.0)
        ap = _alpha([(((-tau) * q["dL"]) / dx, B["hasL"] & (dx < 0)), ((tau * q["dU"]) / dx, B["hasU"] & (dx > 0)),
                     (((-tau) * q["eL"]) / ds_all, B["gL"] & (ds_all < 0)), ((tau * q["eU"]) / ds_all, B["gU"] & (ds_all > 0))])
        ad = _alpha([(((-tau) * zL) / dzL, B["hasL"] & (dzL < 0)), (((-tau) * zU) / dzU, B["hasU"] & (dzU < 0)),
                     (((-tau) * vL) / dvL_all, B["gL"] & (dvL_all < 0)), (((-tau) * vU) / dvU_all, B["gU"] & (dvU_all < 0))])
        # a NaN anywhere in a direction makes its step length +0.0, whatever the bounds
        if np.isnan(sol).any() or np.isnan(ds_all[ine]).any():
            ap = 0.0
        if np.isnan(dzL[B["hasL"]]).any() or np.isnan(dzU[B["hasU"]]).any() or np.isnan(dvL_all[B["gL"]]).any() or np.isnan(dvU_all[B["gU"]]).any():
            ad = 0.0
    dirs = (np.where(ine, ds_all, bufs[0]), dzL, dzU, np.where(ine, dvL_all, bufs[1]), np.where(ine, dvU_all, bufs[2]))
    return dirs, np.array([ap, ad])


def update(B, st, sol, dirs, alpha, mu=MU, kappa=KAPPA):
    """the new state; either step length +0.0: the state as it was"""
    x, s, y, zL, zU, vL, vU = st
    ds, dzL, dzU, dvL, dvU = dirs
    ap, ad = float(alpha[0]), float(alpha[1])
    if not (ap > 0.0 and ad > 0.0):
        return tuple(a.copy() for a in st)
    nvar = len(x)
    ine = ~B["eq"]
    with np.errstate(all="ignore"):
        guard = lambda z, gap: np.minimum(np.maximum(z, mu / (kappa * gap)), (kappa * mu) / gap)
        xn = x + ap * sol[:nvar]
        yn = y + ap * sol[nvar:]
        sn = np.where(ine, s + ap * ds, s)
        zLn = np.where(B["hasL"], guard(zL + ad * dzL, xn - B["xl"]), zL)
        zUn = np.where(B["hasU"], guard(zU + ad * dzU, B["xu"] - xn), zU)
        vLn = np.where(B["gL"], guard(vL + ad * dvL, sn - B["rl"]), vL)
        vUn = np.where(B["gU"], guard(vU + ad * dvU, B["ru"] - sn), vU)
    return xn, sn, yn, zLn, zUn, vLn, vUn


def _max_abs(a, on=None):
    a = np.abs(a if on is None else a[on])
    with np.errstate(invalid="ignore"):
        return float(a.max()) if a.size else 0.0      # (numpy's max propagates a NaN, as the maximum on the bit patterns does)


def merit_terms(B, x, s, c):
    """the addends of theta and of sum log gap"""
    with np.errstate(all="ignore"):
        inf = np.where(B["eq"], c - B["ceq"], c - s)
        logs = np.concatenate([np.log((x - B["xl"])[B["hasL"]]), np.log((B["xu"] - x)[B["hasU"]]), np.log((s - B["rl"])[B["gL"]]), np.log((B["ru"] - s)[B["gU"]])])
    return np.abs(inf), logs


def error(B, st, r, c, mu=MU):
    """``(out[0..3] exactly, [terms of out[4]], ... [terms of out[7]])``; r = None: out[0] is NaN"""
    x, s, y, zL, zU, vL, vU = st
    ine = ~B["eq"]
    q = _side(B, st, mu)
    with np.errstate(all="ignore"):
        t = r if r is not None else np.zeros_like(x)
        t = np.where(B["hasL"], t - zL, t)
        t = np.where(B["hasU"], t + zU, t)
        u = -y
        u = np.where(B["gL"], u - vL, u)
        u = np.where(B["gU"], u + vU, u)
        inf = np.where(B["eq"], c - B["ceq"], c - s)
        comp = np.concatenate([(q["dL"] * zL - mu)[B["hasL"]], (q["dU"] * zU - mu)[B["hasU"]], (q["eL"] * vL - mu)[B["gL"]], (q["eU"] * vU - mu)[B["gU"]]])
    head = np.array([_max_abs(t) if r is not None else NAN, _max_abs(u, ine), _max_abs(inf), _max_abs(comp)])
    mult = np.concatenate([zL[B["hasL"]], zU[B["hasU"]], vL[B["gL"]], vU[B["gU"]]])
    theta, logs = merit_terms(B, x, s, c)
    return head, np.abs(y), mult, theta, logs


def sum_bound(terms):
    """``(math.fsum(terms), (N + 2)·2⁻⁵²·Σ|term|)``: the bound of any summation order of N terms, plus one ulp each for the device's and
    numpy's log"""
    terms = np.asarray(terms, dtype=np.float64)
    return math.fsum(terms), (len(terms) + 2) * 2.0 ** -52 * math.fsum(np.abs(terms))


_points = {}


def barrier_point(name, seed=0):
    """The shared test state of a model, built once per (name, seed) and left unchanged: dict(core, blob, om, B, lvar, uvar, lcon,
    ucon, state = (x, s, y, zL, zU, vL, vU), r, c, mu, tau, relax).  Strictly interior: two-sided entries at lo + U(0.05, 0.95)·(hi − lo),
    one-sided entries 10^U(−2, 1) off their bound, free entries from cases.eval_point_for; multipliers 10^U(−2, 2) where present, NaN
    where absent; NaN on every equality row of s, vL, vU.  r = grad f + J'y and c at x from the oracle."""
    if (name, seed) in _points:
        return _points[name, seed]
    import cases
    from pyoracle import OracleModel
    core = cases.build_core(name)
    blob = core.to_blob()
    om = OracleModel(blob)
    lvar, uvar, lcon, ucon = om.lvar, om.uvar, om.lcon, om.ucon
    B = relaxed_bounds(lvar, uvar, lcon, ucon, RELAX)
    rng = np.random.default_rng(1000 + seed)
    x, y = cases.eval_point_for(name, om, seed)

    def inside(v, lo, hi, has_lo, has_hi):
        both = has_lo & has_hi
        with np.errstate(invalid="ignore"):
            v = np.where(both, lo + rng.uniform(0.05, 0.95, len(v)) * (hi - lo), v)
            v = np.where(has_lo & ~has_hi, lo + 10.0 ** rng.uniform(-2.0, 1.0, len(v)), v)
            v = np.where(has_hi & ~has_lo, hi - 10.0 ** rng.uniform(-2.0, 1.0, len(v)), v)
        return v
    x = inside(x, B["xl"], B["xu"], B["hasL"], B["hasU"])
    c = om.cons(x)
    s = np.where(B["eq"], NAN, inside(c.copy(), B["rl"], B["ru"], B["gL"], B["gU"]))
    mult = lambda on: np.where(on, 10.0 ** rng.uniform(-2.0, 2.0, len(on)), NAN)
    zL, zU, vL, vU = mult(B["hasL"]), mult(B["hasU"]), mult(B["gL"]), mult(B["gU"])
    r = om.grad(x) + om.jtprod(x, y)
    P = dict(core=core, blob=blob, om=om, B=B, lvar=lvar, uvar=uvar, lcon=lcon, ucon=ucon, state=(x, s, y, zL, zU, vL, vU), r=r, c=c, mu=MU, tau=TAU, relax=RELAX)
    with np.errstate(invalid="ignore"):
        assert (x > B["xl"]).all() and (x < B["xu"]).all() and ((s > B["rl"]) | B["eq"]).all() and ((s < B["ru"]) | B["eq"]).all()
    _points[name, seed] = P
    return P


def newton_blocks(P, K_parts, sol, dirs, dw, dc, mu=MU):
    """The four blocks of the UNREDUCED (regularised) primal-dual Newton system at P's state, as residual vectors: stationarity in x,
    stationarity in s, linearised constraints, linearised complementarity.  K_parts = (W, J) scipy matrices (W symmetric, full)."""
    W, J = K_parts
    B = P["B"]
    x, s, y, zL, zU, vL, vU = P["state"]
    ds, dzL, dzU, dvL, dvU = dirs
    nvar = len(x)
    dx, dy = sol[:nvar], sol[nvar:]
    ine = ~B["eq"]
    z = lambda a, on: np.where(on, a, 0.0)
    with np.errstate(all="ignore"):
        b1 = (W @ dx + dw * dx + J.T @ dy - z(dzL, B["hasL"]) + z(dzU, B["hasU"])) + (P["r"] - z(zL, B["hasL"]) + z(zU, B["hasU"]))
        b2 = z((-dy - z(dvL, B["gL"]) + z(dvU, B["gU"])) + (-y - z(vL, B["gL"]) + z(vU, B["gU"])), ine)
        b3 = (J @ dx - z(ds, ine) - dc * dy) + np.where(B["eq"], P["c"] - B["ceq"], P["c"] - s)
        b4 = np.concatenate([(zL * dx + (x - B["xl"]) * dzL - (mu - (x - B["xl"]) * zL))[B["hasL"]], (-zU * dx + (B["xu"] - x) * dzU - (mu - (B["xu"] - x) * zU))[B["hasU"]],
                             (vL * ds + (s - B["rl"]) * dvL - (mu - (s - B["rl"]) * vL))[B["gL"]], (-vU * ds + (B["ru"] - s) * dvU - (mu - (B["ru"] - s) * vU))[B["gU"]]])
    return b1, b2, b3, b4


def oracle_matrices(om, x, y, w=1.0):
    """``(W, J)``: the symmetric Hessian of the Lagrangian and the Jacobian from the oracle's values"""
    import scipy.sparse as sp
    n, m = om.nvar, om.ncon
    hr, hc = om.hess_structure()
    jr, jc = om.jac_structure()
    L = sp.coo_matrix((om.hess_coord(x, y, w), (hr, hc)), shape=(n, n)).tocsr()
    return (L + L.T - sp.diags(L.diagonal())).tocsr(), sp.coo_matrix((om.jac_coord(x), (jr, jc)), shape=(m, n)).tocsr()
