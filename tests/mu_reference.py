"""numpy restatement of csrc/iem_mu_device.h — the twelve words of mu_error and mu_update block in, block out, expression for
expression (numpy rounds every operation and contracts nothing: what -ffp-contract=off makes of the kernels) — on top of
tests/barrier_reference.py.  TEST INFRASTRUCTURE: tests/test_mu.py (CPU), tests/test_gpu_mu.py, tests/mu_loop.py.

The block is a float64 array of sixteen words; words 8–11 hold int64 bit patterns (``ints(blk)`` is the int64 view)."""
import numpy as np

import barrier_reference as bref

ITERATING, CONVERGED, UNUSABLE = 0, 1, 2
MAX_DECREASES = 64
OPTS = dict(mu_init=0.1, kappa_eps=10.0, kappa_mu=0.2, tau_min=0.99, tol=1e-8, mu_floor=0.0, s_max=100.0)
F = np.float64


def options(**over):
    """the options as iem_mu_create resolves them: mu_floor = 0 becomes max(1e-11, tol/10)"""
    o = {**OPTS, **over}
    if o["mu_floor"] == 0.0:
        o["mu_floor"] = max(1e-11, o["tol"] / 10.0)
    return o


def ints(blk):
    return blk.view(np.int64)


def fresh_block(opts, mu0=None):
    """the block behind iem_mu_create / a reset to mu0"""
    blk = np.zeros(16)
    mu = F(opts["mu_init"] if mu0 is None else mu0)
    blk[0], blk[1], blk[2] = mu, np.maximum(F(opts["tau_min"]), F(1.0) - mu), np.sqrt(mu)
    return blk


def reset(blk, opts, mu0):
    """mu_reset: words 0–2 from mu0, words 8–11 zero, words 3–7 stay"""
    out = blk.copy()
    out[:3] = fresh_block(opts, mu0)[:3]
    ints(out)[8:12] = 0
    return out


def products(B, st):
    """the complementarity products gap·z over the present bounds, each rounded once (the order: xL, xU, sL, sU — the extremes and the
    count do not depend on it)"""
    x, s, y, zL, zU, vL, vU = st
    with np.errstate(all="ignore"):
        return np.concatenate([((x - B["xl"]) * zL)[B["hasL"]], ((B["xu"] - x) * zU)[B["hasU"]], ((s - B["rl"]) * vL)[B["gL"]], ((B["ru"] - s) * vU)[B["gU"]]])


def enters(p):
    """the products that are >= +0.0: sign bit clear and not a NaN (−0.0 does not enter)"""
    return p.view(np.uint64) <= np.uint64(0x7ff0000000000000)


def error_words(B, st, r, c):
    """``(head, sums, w8, w10, p)``: words 0–3 exactly, the terms of words 4–7 as barrier_reference.error gives them, word 8, word 10
    and the products (the terms of word 9)"""
    head, ay, mult, theta, logs = bref.error(B, st, r, c, 0.0)
    p = products(B, st)
    ok = enters(p)
    w8 = float(p[ok].min()) if ok.any() else float("inf")
    return head, (ay, mult, theta, logs), w8, float((~ok).sum()), p


def product_addends(B, st):
    """the products over [0, nvar + ncon) in mu_error's statement order: ``(pL, pU)`` — lower then upper on a variable and on an
    inequality row, +0.0 where the bound is absent — and the masks of the present bounds laid out the same way"""
    x, s, y, zL, zU, vL, vU = st
    with np.errstate(all="ignore"):
        pL = bref.full(B, B["hasL"], (x - B["xl"]) * zL, B["gL"], (s - B["rl"]) * vL)
        pU = bref.full(B, B["hasU"], (B["xu"] - x) * zU, B["gU"], (B["ru"] - s) * vU)
    return (pL, pU), (np.concatenate([B["hasL"], B["gL"]]), np.concatenate([B["hasU"], B["gU"]]))


def product_sums(B, st, n_wg):
    """``(word 9, word 10)`` of mu_error on a grid of `n_wg` workgroups, in the device's order: the sum of the products and the count
    of those that do not enter the minimum"""
    (pL, pU), (onL, onU) = product_addends(B, st)
    bad = [np.where(on, ~enters(np.ascontiguousarray(p)), False).astype(np.float64) for p, on in ((pL, onL), (pU, onU))]
    return bref.device_sum([pL, pU], n_wg), bref.device_sum(bad, n_wg)


def terms(w, counts, opts):
    """``(e_d, e_p, sc)`` of mu_update from the twelve words"""
    m, nz = int(counts[0]), int(counts[1])
    w = np.asarray(w, dtype=np.float64)
    s_max = F(opts["s_max"])
    with np.errstate(all="ignore"):
        sd = np.maximum(s_max, (w[4] + w[5]) / F(max(1, m + nz))) / s_max
        sc = np.maximum(s_max, w[5] / F(max(1, nz))) / s_max
        e_d = np.maximum(w[0], w[1]) / sd
    e_p = w[2] if m else F(0.0)
    return e_d, e_p, sc


def e_c(w, counts, sc, mu):
    with np.errstate(all="ignore"):
        return np.maximum(w[3] - mu, mu - w[8]) / sc if int(counts[1]) else F(0.0)


def E(w, counts, opts, mu):
    """Ipopt's scaled optimality error at mu from the twelve words"""
    w = np.asarray(w, dtype=np.float64)
    e_d, e_p, sc = terms(w, counts, opts)
    return np.maximum(np.maximum(e_d, e_p), e_c(w, counts, sc, F(mu)))


def update(blk, w, counts, opts, ctl=None):
    """mu_update: ``(block, ctl)`` after the call — ctl a search's control block (16 words) or None"""
    w = np.asarray(w, dtype=np.float64)
    blk = blk.copy()
    ctl = None if ctl is None else ctl.copy()
    e_d, e_p, sc = terms(w, counts, opts)
    Emu = lambda mu: np.maximum(np.maximum(e_d, e_p), e_c(w, counts, sc, mu))
    mu = F(blk[0])
    floor, kappa_eps, kappa_mu = F(opts["mu_floor"]), F(opts["kappa_eps"]), F(opts["kappa_mu"])
    e0, ec0 = Emu(F(0.0)), e_c(w, counts, sc, F(0.0))
    k = 0
    if w[10] != 0.0 or np.isnan(e0):
        status = UNUSABLE
    elif e0 <= opts["tol"]:
        status = CONVERGED
    else:
        status = ITERATING
        while mu > floor and Emu(mu) <= kappa_eps * mu and k < MAX_DECREASES:
            mu = np.maximum(floor, np.minimum(kappa_mu * mu, mu * np.sqrt(mu)))
            k += 1
    iw = ints(blk)
    if k > 0:
        blk[0], blk[1], blk[2] = mu, np.maximum(F(opts["tau_min"]), F(1.0) - mu), np.sqrt(mu)
        iw[9] |= 1
        iw[10] += k
        if ctl is not None:
            ctl[11] = ctl[12] = 0.0
    else:
        iw[9] &= ~1
    blk[3], blk[4], blk[5], blk[6], blk[7] = e0, Emu(mu), e_d, e_p, ec0
    iw[8] = status
    iw[11] += 1
    return blk, ctl


def central_state(P, mu, spread=0.0, seed=0):
    """P's state with the multipliers on the central path: z = mu/gap (times 1 + spread·U(−1, 1)) wherever a bound is present"""
    B = P["B"]
    x, s, y, zL, zU, vL, vU = P["state"]
    rng = np.random.default_rng(seed)
    j = lambda n: 1.0 + spread * rng.uniform(-1.0, 1.0, n)
    with np.errstate(all="ignore"):
        return (x, s, y, np.where(B["hasL"], mu / (x - B["xl"]) * j(len(x)), zL), np.where(B["hasU"], mu / (B["xu"] - x) * j(len(x)), zU),
                np.where(B["gL"], mu / (s - B["rl"]) * j(len(s)), vL), np.where(B["gU"], mu / (B["ru"] - s) * j(len(s)), vU))


def feasible(P):
    """P with r and c of a point that is dual and primal feasible: only complementarity is left in the error"""
    B = P["B"]
    x, s, y, zL, zU, vL, vU = P["state"]
    z = lambda a, on: np.where(on, a, 0.0)
    Q = dict(P)
    Q["c"] = np.where(B["eq"], B["ceq"], s)
    Q["r"] = z(zL, B["hasL"]) - z(zU, B["hasU"])
    return Q


def branch_cases(name):
    """``(label, P, state, block, opts, expected k)`` — expected: an int, ">=3", or None where only the status matters"""
    P = bref.barrier_point(name)
    opts = options()
    out = [("far from the path", P, P["state"], fresh_block(opts), opts, 0)]
    fe = feasible(P)
    B = P["B"]
    # on the central path of mu = 0.1, dual and primal feasible up to y: the multipliers of the slack side fix y
    for label, mu_c, spread, mu0, o, want in (("one decrease", 0.1, 0.3, 0.1, options(kappa_eps=1.0, kappa_mu=1e-6), 1),
                                              ("several decreases", 1e-7, 0.0, 0.1, opts, ">=3"),
                                              ("stop at the floor", 1e-13, 0.0, 1e-9, options(tol=1e-14, mu_floor=1e-10), None),
                                              ("converged", 1e-12, 0.0, 0.1, opts, 0)):
        st = list(central_state(fe, mu_c, spread, seed=3))
        with np.errstate(invalid="ignore"):
            st[2] = np.where(B["eq"], st[2], np.where(B["gU"], st[6], 0.0) - np.where(B["gL"], st[5], 0.0))      # -y - vL + vU = 0
        Q = feasible(dict(fe, state=tuple(st)))
        out.append((label, Q, tuple(st), fresh_block(o, mu0), o, want))
    bad = [a.copy() for a in P["state"]]
    i = int(np.flatnonzero(B["hasL"] | B["hasU"])[0])
    (bad[3] if B["hasL"][i] else bad[4])[i] = np.nan
    out.append(("a NaN multiplier", P, tuple(bad), fresh_block(opts), opts, 0))
    neg = [a.copy() for a in P["state"]]
    (neg[3] if B["hasL"][i] else neg[4])[i] = -1.0
    out.append(("a negative product", P, tuple(neg), fresh_block(opts), opts, 0))
    return out
