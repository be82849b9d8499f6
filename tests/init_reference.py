"""numpy restatement of csrc/iem_init_device.h — init_ls_terms, init_ls_norm / init_ls_apply, init_warm, init_mu — block in, block
out, expression for expression (numpy rounds every operation and contracts nothing: what -ffp-contract=off makes of the kernels),
on top of tests/barrier_reference.py and tests/mu_reference.py.  TEST INFRASTRUCTURE: tests/test_init.py (CPU),
tests/test_gpu_init.py, tests/init_loop.py.

The own block is a float64 array of sixteen words; words 1–3 and 5 hold int64 bit patterns (``ints(blk)`` is the int64 view).
Vectors are full length; where the kernels branch on a presence flag the restatement computes on every entry and selects with
np.where: the selected entries carry the same bits.  Entries of s, vL, vU on equality rows pass through untouched.

The host side of the least-squares estimate (`dense_jacobian`, `ls_system`, `ls_solve`, `ls_lstsq`, `ls_objective`, `cold_point`) is
dense numpy around the restated kernels: what tests/test_init.py holds against numpy.linalg.lstsq."""
import numpy as np

import barrier_reference as bref
import mu_reference as mref

YNORM, ACCEPTED, N_ACCEPTED, N_REJECTED, MU0, HOW = range(6)
FROM_AVERAGE, FALLBACK, CLAMPED_BELOW, CLAMPED_ABOVE = range(4)
OPTS = dict(y_max=1e3, on_reject=0, warm_push=1e-3, warm_frac=1e-3, warm_z_push=1e-3, warm_z_max=1e6, warm_y_max=1e6, mu_factor=1.0, mu_cap=0.0)
F = np.float64


def options(**over):
    unknown = set(over) - set(OPTS)
    assert not unknown, unknown
    return {**OPTS, **over}


def ints(blk):
    return blk.view(np.int64)


def fresh_block():
    """the block behind iem_init_create / iem_init_reset"""
    return np.zeros(16)


# ---- init_ls_terms ----------------------------------------------------------------------------------------------------------------------
def ls_terms(B, st, r):
    """``(sigma, dcon, rhs)``: every entry is written"""
    x, s, y, zL, zU, vL, vU = st
    with np.errstate(all="ignore"):
        sigma = np.full(len(r), 1.0)
        a = np.where(B["hasL"], r - zL, r)
        a = np.where(B["hasU"], a + zU, a)
        rhs_x = -a
        tl = np.where(B["gL"], vL, 0.0)
        tu = np.where(B["gU"], vU, 0.0)
        t = tl - tu
        dcon = np.where(B["eq"], 0.0, 1.0)
        rhs_y = np.where(B["eq"], 0.0, y + t)
    return sigma, dcon, np.concatenate([rhs_x, rhs_y])


# ---- init_ls_norm, init_ls_apply --------------------------------------------------------------------------------------------------------
def ls_norm(y, sol, nvar):
    """``(yn, ynorm)``: yn = y + sol[nvar:], ynorm the integer maximum on the bit patterns of |yn| (a NaN wins; no rows: +0.0)"""
    with np.errstate(all="ignore"):
        yn = y + sol[nvar:]
    top = np.abs(yn).view(np.uint64).max() if len(yn) else np.uint64(0)
    return yn, np.array([top], dtype=np.uint64).view(np.float64)[0]


def ls_apply(blk, y, sol, nvar, opts):
    """``(block, y)`` after iem_init_ls_apply; sol's x part is never read"""
    blk = blk.copy()
    yn, ynorm = ls_norm(y, sol, nvar)
    with np.errstate(invalid="ignore"):
        accepted = bool(ynorm <= F(opts["y_max"]))      # a NaN compares false
    iw = ints(blk)
    blk[YNORM] = ynorm
    iw[ACCEPTED] = int(accepted)
    iw[N_ACCEPTED] += int(accepted)
    iw[N_REJECTED] += int(not accepted)
    if accepted:
        return blk, yn
    return blk, (y.copy() if opts["on_reject"] else np.zeros(len(y)))


# ---- init_warm --------------------------------------------------------------------------------------------------------------------------
def clamp(z, on, lo, hi):
    """a present multiplier: at least lo (a NaN becomes lo), at most hi; an absent one: +0.0"""
    with np.errstate(invalid="ignore"):
        z = np.where(z > lo, z, lo)
        z = np.where(z < hi, z, hi)
    return np.where(on, z, 0.0)


def warm(B, st, opts):
    """``(x, s, y, zL, zU, vL, vU)`` after iem_init_warm; s, vL, vU on equality rows as they were"""
    x, s, y, zL, zU, vL, vU = st
    ine = ~B["eq"]
    k1, k2, zp, zm, ym = (F(opts[k]) for k in ("warm_push", "warm_frac", "warm_z_push", "warm_z_max", "warm_y_max"))
    xw = bref.push(x, B["xl"], B["xu"], B["hasL"], B["hasU"], k1, k2)
    sw = np.where(ine, bref.push(s, B["rl"], B["ru"], B["gL"], B["gU"], k1, k2), s)
    with np.errstate(invalid="ignore"):
        yw = np.where(np.isnan(y), 0.0, np.where(y < -ym, -ym, np.where(y > ym, ym, y)))
    return (xw, sw, yw, clamp(zL, B["hasL"], zp, zm), clamp(zU, B["hasU"], zp, zm), np.where(ine, clamp(vL, B["gL"], zp, zm), vL),
            np.where(ine, clamp(vU, B["gU"], zp, zm), vU))


# ---- init_mu ----------------------------------------------------------------------------------------------------------------------------
def choose_mu(w, nz, opts, mu_opts):
    """``(mu0, how)`` from the twelve words of mu_error; mu_opts: the RESOLVED options of the iem_mu object (mu_reference.options)"""
    w = np.asarray(w, dtype=np.float64)
    nz = int(nz)
    mu_init, floor = F(mu_opts["mu_init"]), F(mu_opts["mu_floor"])
    cap = F(opts["mu_cap"]) if opts["mu_cap"] != 0.0 else mu_init
    if nz == 0 or w[10] != 0.0:
        return mu_init, FALLBACK
    with np.errstate(all="ignore"):
        avg = w[9] / F(nz)
        if not avg > 0.0:      # a NaN compares false
            return mu_init, FALLBACK
        t = F(opts["mu_factor"]) * avg
    mu0, how = t, FROM_AVERAGE
    if t > cap:
        mu0, how = cap, CLAMPED_ABOVE
    if mu0 < floor:
        mu0, how = floor, CLAMPED_BELOW
    return mu0, how


def mu(blk, mu_blk, w, nz, opts, mu_opts):
    """``(block, mu block)`` after iem_init_mu: words 0–2 and 8–11 of the iem_mu block as mu_reference.reset writes them at mu0"""
    blk = blk.copy()
    mu0, how = choose_mu(w, nz, opts, mu_opts)
    blk[MU0] = mu0
    ints(blk)[HOW] = how
    return blk, mref.reset(mu_blk, mu_opts, mu0)


# ---- the host side of the estimate (dense) ------------------------------------------------------------------------------------------------
def dense_jacobian(om, x):
    """J (ncon × nvar) from the structure and value calls of the oracle; duplicate entries add"""
    rows, cols = om.jac_structure()
    J = np.zeros((om.ncon, om.nvar))
    np.add.at(J, (np.asarray(rows), np.asarray(cols)), om.jac_coord(x))
    return J


def ls_system(J, sigma, dcon, delta_c=0.0):
    """the K of the estimate, dense: a zero Hessian, delta_w = 0 — [diag(sigma), J'; J, −diag(dcon + delta_c)]"""
    m, n = J.shape
    K = np.zeros((n + m, n + m))
    K[:n, :n] = np.diag(sigma)
    K[:n, n:] = J.T
    K[n:, :n] = J
    K[n:, n:] = -np.diag(dcon + delta_c)
    return K


def ls_solve(B, st, r, J, delta_c=0.0):
    """``sol = [w; delta]`` of the K built from ls_terms' output"""
    sigma, dcon, rhs = ls_terms(B, st, r)
    return np.linalg.solve(ls_system(J, sigma, dcon, delta_c), rhs)


def ls_stacked(B, st, r, J):
    """``(A, b)`` of the stacked problem  min ‖A delta + b‖₂:  [J'; −E] delta + [r − zL + zU; −y − vL + vU], E the inequality rows of I"""
    x, s, y, zL, zU, vL, vU = st
    z = lambda a, on: np.where(on, a, 0.0)
    ine = ~B["eq"]
    E = np.eye(len(y))[ine]
    A = np.vstack([J.T, -E])
    b = np.concatenate([r - z(zL, B["hasL"]) + z(zU, B["hasU"]), (-y - z(vL, B["gL"]) + z(vU, B["gU"]))[ine]])
    return A, b


def ls_lstsq(B, st, r, J):
    """numpy's two routes to the minimiser of the stacked problem: ``(lstsq (SVD), the normal equations A'A delta = −A'b)``"""
    A, b = ls_stacked(B, st, r, J)
    return np.linalg.lstsq(A, -b, rcond=None)[0], np.linalg.solve(A.T @ A, -(A.T @ b))


def ls_objective(B, st, r, J, delta):
    A, b = ls_stacked(B, st, r, J)
    v = A @ delta + b
    return float(v @ v)


def cold_point(om, relax=bref.RELAX):
    """``(B, state, r, J)`` of a cold start at the oracle's x0: barrier_reference.start, y = 0, r = the gradient at the pushed point"""
    B = bref.relaxed_bounds(om.lvar, om.uvar, om.lcon, om.ucon, relax)
    m = om.ncon
    x0 = np.asarray(om.x0, dtype=np.float64)
    bufs = tuple(np.full(m, bref.NAN) for _ in range(3))
    x = bref.push(x0, B["xl"], B["xu"], B["hasL"], B["hasU"])
    x, s, zL, zU, vL, vU = bref.start(B, x, om.cons(x), bufs)
    y = np.zeros(m)
    return B, (x, s, y, zL, zU, vL, vU), om.grad(x), dense_jacobian(om, x)
