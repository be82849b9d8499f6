"""numpy restatement of csrc/iem_barrier_device.h — barrier_start, barrier_terms, barrier_step, barrier_update, barrier_error,
barrier_merit, expression for expression (numpy rounds every operation and contracts nothing: what -ffp-contract=off makes of the
kernels) — and the state the tests of the barrier layer share.  TEST INFRASTRUCTURE: tests/test_barrier.py (CPU) and
tests/test_gpu_barrier.py.

THE SUMS are restated in the device's order (`device_sum`, shared by every restatement built on this one): a lane adds the addends of
its entries i, i + 256·n_wg, ... one after the other from +0.0, the 64 lanes of a wave meet in the shuffle tree of iem_wave_sum, the
four waves of a workgroup are added in order, and the last arrival totals the column — lane l takes the workgroups l, l + 64, ...,
then the same tree.  `error_sums` / `merit_sums` are bitwise the kernels' for the grid they are given, but for sum log gap (numpy's
log).  `big_point` is the shared state of the shapes at which the stride loop runs more than once (tests/test_device_order.py, CPU).

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


def _tree(a):
    """iem_wave_sum on the last axis (64 lanes): what lane 0 holds"""
    a = a.copy()
    for off in (32, 16, 8, 4, 2, 1):
        a[..., :off] = a[..., :off] + a[..., off:2 * off]
    return a[..., 0]


def device_sum(addends, n_wg):
    """One column of iem_shared_park / iem_shared_totals over a grid of `n_wg` workgroups of 256: `addends` is a list of arrays over
    the entries [0, n) — what a lane adds for entry i, in that order (+0.0 where the kernel adds nothing: the accumulators start
    from +0.0 and never hold −0.0, so the bits are the same).  A lane adds the addends of its entries i, i + 256·n_wg, ... one after
    the other from +0.0, the 64 lanes of a wave meet in the shuffle tree of iem_wave_sum, the four waves of a workgroup are added in
    order, and the last arrival totals the column — lane l takes the workgroups l, l + 64, ..., then the same tree."""
    n_wg = int(n_wg)
    T = 256 * n_wg
    n = len(addends[0])
    acc = np.zeros(T)
    with np.errstate(all="ignore"):
        for k in range(0, n, T):
            for a in addends:
                seg = a[k:k + T]
                acc[:len(seg)] = acc[:len(seg)] + seg
        waves = _tree(acc.reshape(n_wg, 4, 64))
        parked = ((waves[:, 0] + waves[:, 1]) + waves[:, 2]) + waves[:, 3]
        pad = np.zeros(-(-n_wg // 64) * 64)
        pad[:n_wg] = parked
        lanes = np.zeros(64)
        for row in pad.reshape(-1, 64):
            lanes = lanes + row
        return np.float64(_tree(lanes))


def full(B, on_x, vx, on_s, vs):
    """addends over [0, nvar + ncon): vx where on_x, vs where on_s, +0.0 elsewhere (None: nothing on that side)"""
    nvar, ncon = len(B["hasL"]), len(B["eq"])
    with np.errstate(all="ignore"):
        return np.concatenate([np.zeros(nvar) if on_x is None else np.where(on_x, vx, 0.0), np.zeros(ncon) if on_s is None else np.where(on_s, vs, 0.0)])


def grid(n):
    """kkt_stream_grid of csrc/iem_api.cpp: min(ceil(n / 256), 4096) workgroups"""
    return min(-(-int(n) // 256), 4096)


def trips(nvar, n, n_wg):
    """``[(variables, rows), ...]``: how many entries of each branch the grid takes on each trip of the stride loop"""
    T = 256 * int(n_wg)
    return [(max(0, min(k + T, nvar) - k), min(k + T, n) - max(k, nvar) if k + T > nvar else 0) for k in range(0, int(n), T)]


def log_addends(B, x, s):
    """the column `sum log gap` of barrier_error / barrier_merit: lower then upper on a variable and on an inequality row — numpy's
    log, which need not carry the last bit of the device's"""
    with np.errstate(all="ignore"):
        return [full(B, B["hasL"], np.log(x - B["xl"]), B["gL"], np.log(s - B["rl"])), full(B, B["hasU"], np.log(B["xu"] - x), B["gU"], np.log(B["ru"] - s))]


def error_addends(B, st, c):
    """The four parked columns of barrier_error (out[4..7]) as lists of addends over [0, nvar + ncon) in the kernel's statement order:
    sum |y| (every row), the present multipliers (zL then zU on a variable, vL then vU on a row), theta (every row), sum log gap."""
    x, s, y, zL, zU, vL, vU = st
    every = np.ones(len(y), dtype=bool)
    with np.errstate(all="ignore"):
        inf = np.where(B["eq"], c - B["ceq"], c - s)
        return ([full(B, None, None, every, np.abs(y))], [full(B, B["hasL"], zL, B["gL"], vL), full(B, B["hasU"], zU, B["gU"], vU)],
                [full(B, None, None, every, np.abs(inf))], log_addends(B, x, s))


def error_sums(B, st, c, n_wg):
    """out[4..7] of barrier_error on a grid of `n_wg` workgroups: the first three carry the device's bits, the fourth is the device's
    order over numpy's logs"""
    return np.array([device_sum(col, n_wg) for col in error_addends(B, st, c)])


def merit_sums(B, x, s, c, n_wg):
    """the two of barrier_merit: the columns of out[6], out[7] of barrier_error"""
    with np.errstate(all="ignore"):
        inf = np.where(B["eq"], c - B["ceq"], c - s)
    return np.array([device_sum([full(B, None, None, np.ones(len(c), dtype=bool), np.abs(inf))], n_wg), device_sum(log_addends(B, x, s), n_wg)])


HEAVY = (36, 29)      # which candidate lane carries the weight and the seed of its multipliers (chosen so that tests/test_device_order.py passes)
H57 = 2.0 ** 57


def _heavy_lane(P, k, seed):
    """THE SPREAD of the sizes above 27 000 (that one keeps its recipe).  Over 10⁶ addends of one magnitude a total's last bit is
    10⁶ times coarser than a lane's, so no order of a lane's additions shows in it: the bits of a total discriminate only where one
    lane outweighs all the others.  So one lane does — the entries i0, i0 + T, i0 + 2T (T = 4096·256: the same lane on three trips,
    two variables and a row, each with both bounds; the k-th such lane).  Its six multipliers become 2⁵⁷·(1, 1, 2, 4, 8, 16)·U(1, 2)
    in the kernel's order: every addition of the lane lands in another binade, so that the roundings depend on the order (under ONE
    dominating addend the others round on its grid one by one, and their order cannot show).  Returns the three entries; `plant`
    gives a direction (or any vector over the entries) weights there."""
    B, st = P["B"], P["state"]
    n, m = len(st[0]), len(st[2])
    T = 4096 * 256
    assert n > T and n + m > 2 * T
    both_x, both_s = B["hasL"] & B["hasU"], B["gL"] & B["gU"]
    cand = (i for i in range(1000, n - T) if both_x[i] and both_x[i + T] and both_s[i + 2 * T - n])
    for _ in range(k + 1):
        i0 = next(cand)
    j = i0 + 2 * T - n
    z = H57 * np.array([1.0, 1.0, 2.0, 4.0, 8.0, 16.0]) * np.random.default_rng(700 + seed).uniform(1.0, 2.0, 6)
    st[3][i0], st[4][i0], st[3][i0 + T], st[4][i0 + T], st[5][j], st[6][j] = z
    return (i0, i0 + T, i0 + 2 * T)


def plant(P, v, scales, seed=0):
    """a copy of `v` (over the entries, over the variables or over the rows) with scales[k]·U(1, 2) at the k-th of P's heavy entries;
    P without them: `v` itself"""
    if P["heavy"] is None:
        return v
    n, m = len(P["state"][0]), len(P["state"][2])
    rng = np.random.default_rng(900 + seed)
    v = v.copy()
    for i, scale in zip(P["heavy"], scales):
        j = i - n if len(v) == m else i
        w = scale * rng.uniform(1.0, 2.0)
        if 0 <= j < len(v):
            v[j] = w
    return v


def cut(B, iv, ir):
    """the bounds dictionary over the variables `iv` and the rows `ir` alone (index arrays): what an order-free word — a maximum, a
    minimum, a step length — takes from those entries is the restatement's value on the cut, at the cost of a few entries"""
    nvar = len(B["hasL"])
    C = {k: (v[iv] if len(v) == nvar else v[ir]) for k, v in B.items() if k != "counts"}
    C["counts"] = dict(nvar=len(iv), ncon=len(ir))
    return C


def cut_state(st, iv, ir):
    return (st[0][iv], st[1][ir], st[2][ir], st[3][iv], st[4][iv], st[5][ir], st[6][ir])


def seam_positions(nvar, n, n_wg):
    """the entries at which a later trip, or the other branch, begins or ends: either side of the nvar seam, 2²⁰ − 1 and 2²⁰ (the last
    entry of the first trip of 4096 workgroups and the first of the second), the first entry of the third trip where there is one,
    and n − 1"""
    T = 256 * int(n_wg)
    pos = {"left of the seam": nvar - 1, "right of the seam": nvar, "2^20 - 1": 2 ** 20 - 1, "2^20": 2 ** 20, "n - 1": n - 1}
    if n > 2 * T:
        pos["first of trip three"] = 2 * T
    assert T == 2 ** 20 and all(0 <= i < n for i in pos.values())
    return pos


def nearest(mask, i):
    """the entry nearest to i at which `mask` (over the entries) holds"""
    idx = np.flatnonzero(mask)
    return int(idx[np.argmin(np.abs(idx - i))])


_big = {}


def big_point(supports=27_000):
    """quadrotor(supports) with bounds and a state of the tests' own, built once per size and left unchanged: variables free / lower /
    upper / both, rows equality / lower / upper / both in equal shares; gaps 10^U(−2, 1), multipliers 10^U(−2, 2), NaN where a bound is
    absent and on equality rows of the slack side; r and c random.  27 000: nvar + ncon = 1 080 000 > 2²⁰ entries, the later trip of
    the stride loop is rows only; 60 000: nvar = 1 320 000 > 2²⁰, three trips, the second crosses the nvar seam."""
    supports = int(supports)
    if supports in _big:
        return _big[supports]
    from infiniteexamodels.jl_amd import transcribe, workloads
    core = transcribe.exa_core(workloads.quadrotor(supports))
    n, m = int(core.nvar), int(core.ncon)
    assert n + m > 2 ** 20
    rng = np.random.default_rng(supports // 10)
    gap = lambda k: 10.0 ** rng.uniform(-2.0, 1.0, k)
    x, kx = rng.standard_normal(n), rng.integers(0, 4, n)
    lvar, uvar = np.where(kx & 1, x - gap(n), -np.inf), np.where(kx & 2, x + gap(n), np.inf)
    s0, kc = rng.standard_normal(m), rng.integers(0, 4, m)
    eq = kc == 0
    lcon, ucon = np.where(eq, s0, np.where(kc & 1, s0 - gap(m), -np.inf)), np.where(eq, s0, np.where(kc & 2, s0 + gap(m), np.inf))
    B = relaxed_bounds(lvar, uvar, lcon, ucon, RELAX)
    mult = lambda on: np.where(on, 10.0 ** rng.uniform(-2.0, 2.0, len(on)), NAN)
    state = (x, np.where(eq, NAN, s0), rng.standard_normal(m), mult(B["hasL"]), mult(B["hasU"]), mult(B["gL"]), mult(B["gU"]))
    P = dict(core=core, blob=None, B=B, lvar=lvar, uvar=uvar, lcon=lcon, ucon=ucon, state=state, r=rng.standard_normal(n), c=s0 + 0.1 * rng.standard_normal(m), mu=MU,
             tau=TAU, relax=RELAX, heavy=None)
    assert B["counts"]["nz"] > 10 ** 5 and B["counts"]["n_eq"] > 10 ** 4
    if supports != 27_000:
        P["heavy"] = _heavy_lane(P, *HEAVY)
    _big[supports] = P
    return P


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
