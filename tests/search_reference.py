"""numpy restatement of csrc/iem_search_device.h — search_begin, search_trial, search_accept, expression for expression (every
operation on IEEE doubles, rounded once, nothing contracted: what -ffp-contract=off makes of the kernels; pow is np.power) — and the
table of hand-built acceptance cases the CPU and the GPU test share.  TEST INFRASTRUCTURE: tests/test_search.py (CPU) and
tests/test_gpu_search.py.  Bounds are the dictionary of barrier_reference.relaxed_bounds.

The control block is a float64 array of 16 words; words 9–12 are int64 (word / set_word read and write them through a view)."""
import math

import numpy as np

import barrier_reference as bref

SEARCHING, F_TYPE, H_TYPE, FAILED, UNUSABLE = 0, 1, 2, 3, 4
ALPHA, ALPHA_MAX, PHI0, THETA0, SLOPE, THETA_MIN, THETA_MAX, PHI_T, THETA_T, STATUS, TRIALS, COUNT, FLAGS = range(13)
OPTS = dict(gamma_theta=1e-5, gamma_phi=1e-8, eta_phi=1e-8, delta=1.0, s_theta=1.1, s_phi=2.3, alpha_floor=1e-16, max_trials=30, filter_capacity=64)
ARMIJO_SLACK = 10.0 * 2.0 ** -52
NAN = float("nan")
SPREAD, SPREAD_SEED = (2.0 ** 20, 2.0 ** 21, 2.0 ** 22), 6      # barrier_reference.plant's weights on the heavy lane of a big shape's direction: the slope discriminates


def word(ctl, w):
    return int(ctl.view(np.int64)[w])


def set_word(ctl, w, v):
    ctl.view(np.int64)[w] = v


def block(**kw):
    """a control block from names: block(alpha=1.0, status=SEARCHING, ...); unnamed words are zero"""
    names = dict(alpha=ALPHA, alpha_max=ALPHA_MAX, phi0=PHI0, theta0=THETA0, slope=SLOPE, theta_min=THETA_MIN, theta_max=THETA_MAX, phi_t=PHI_T, theta_t=THETA_T)
    ints = dict(status=STATUS, trials=TRIALS, count=COUNT, flags=FLAGS)
    ctl = np.zeros(16)
    for k, v in kw.items():
        if k in names:
            ctl[names[k]] = v
        else:
            set_word(ctl, ints[k], v)
    return ctl


def slope_terms(B, x, s, g, sol, ds, mu, sigma=1.0):
    """the addends of the slope in index order: (sigma·g_i + gb_i)·dx_i per variable, then gs_j·ds_j per inequality row"""
    nvar = len(x)
    dx = sol[:nvar]
    ine = ~B["eq"]
    with np.errstate(all="ignore"):
        ml, mu_u = np.where(B["hasL"], mu / (x - B["xl"]), 0.0), np.where(B["hasU"], mu / (B["xu"] - x), 0.0)
        tx = (sigma * g + (mu_u - ml)) * dx
        nl, nu = np.where(B["gL"], mu / (s - B["rl"]), 0.0), np.where(B["gU"], mu / (B["ru"] - s), 0.0)
        ts = ((nu - nl) * ds)[ine]
    return np.concatenate([tx, ts])


def slope_addends(B, x, s, g, sol, ds, mu, sigma=1.0):
    """the one parked column of search_begin over [0, nvar + ncon): (sigma·g_i + gb_i)·dx_i on a variable, gs_j·ds_j on an inequality
    row, nothing (+0.0) on an equality row — one addend per entry"""
    nvar = len(x)
    with np.errstate(all="ignore"):
        ml, mu_u = np.where(B["hasL"], mu / (x - B["xl"]), 0.0), np.where(B["hasU"], mu / (B["xu"] - x), 0.0)
        nl, nu = np.where(B["gL"], mu / (s - B["rl"]), 0.0), np.where(B["gU"], mu / (B["ru"] - s), 0.0)
        return [bref.full(B, np.ones(nvar, dtype=bool), (sigma * g + (mu_u - ml)) * sol[:nvar], ~B["eq"], (nu - nl) * ds)]


def slope(B, x, s, g, sol, ds, mu, sigma, n_wg):
    """the slope search_begin sums on a grid of `n_wg` workgroups: the device's bits (barrier_reference.device_sum)"""
    return bref.device_sum(slope_addends(B, x, s, g, sol, ds, mu, sigma), n_wg)


_big = {}


def big_inputs(supports):
    """host side of a search at barrier_reference.big_point(supports), built once per size: ``(g, sol, ds, f, alpha)`` — random, NaN
    in ds on equality rows (never read), and barrier_reference.plant's weights on the heavy lane of the direction"""
    if supports not in _big:
        P = bref.big_point(supports)
        B = P["B"]
        n, m = len(P["state"][0]), len(P["state"][2])
        rng = np.random.default_rng(77)
        g, sol, ds = rng.standard_normal(n), rng.standard_normal(n + m), np.where(B["eq"], NAN, rng.standard_normal(m))
        _big[supports] = (g, bref.plant(P, sol, SPREAD, SPREAD_SEED), bref.plant(P, ds, SPREAD, SPREAD_SEED), 1.25, np.array([0.75, 0.5]))
    return _big[supports]


def begin(ctl, slope, obj, err, alpha, mu, sigma=1.0):
    """the block search_begin's last workgroup leaves, given the slope it summed; the count and flag bit 1 stay"""
    ctl = ctl.copy()
    slope, amax, theta0 = float(slope), float(alpha[0]), float(err[6])
    usable = amax > 0.0 and slope == slope
    ctl[ALPHA] = amax if usable else 0.0
    ctl[ALPHA_MAX] = amax
    ctl[PHI0] = sigma * float(obj) - mu * float(err[7])
    ctl[THETA0] = theta0
    ctl[SLOPE] = slope
    flags = word(ctl, FLAGS)
    if not flags & 1:
        t1 = theta0 if theta0 > 1.0 else 1.0
        ctl[THETA_MIN] = 1e-4 * t1
        ctl[THETA_MAX] = 1e4 * t1
        set_word(ctl, FLAGS, flags | 1)
    ctl[PHI_T] = ctl[THETA_T] = NAN
    set_word(ctl, STATUS, SEARCHING if usable else UNUSABLE)
    set_word(ctl, TRIALS, 0)
    ctl[13:] = 0.0
    return ctl


def trial(B, ctl, x, s, sol, ds, bufs):
    """``(xt, st)``; bufs = (xt, st) as they were: equality rows' entries of st stay, and everything stays under FAILED / UNUSABLE"""
    if word(ctl, STATUS) in (FAILED, UNUSABLE):
        return bufs[0].copy(), bufs[1].copy()
    a = float(ctl[ALPHA])
    with np.errstate(all="ignore"):
        return x + a * sol[:len(x)], np.where(~B["eq"], s + a * ds, bufs[1])


def accept(ctl, filt, ft, merit, mu, sigma=1.0, opts=OPTS, info=None):
    """search_accept: ``(control block, filter, d_alpha[0])``; `filt`: (capacity, 2) array of (theta, phi), the first `count` rows in
    use.  `info` (a dict) receives the two sides of the switching condition's comparison when it was evaluated."""
    ctl, filt = ctl.copy(), filt.copy()
    status = word(ctl, STATUS)
    if status != SEARCHING:
        return ctl, filt, float(ctl[ALPHA]) if status in (F_TYPE, H_TYPE) else 0.0
    alpha, phi0, theta0, slope, theta_min, theta_max = (float(ctl[w]) for w in (ALPHA, PHI0, THETA0, SLOPE, THETA_MIN, THETA_MAX))
    trials, flags = word(ctl, TRIALS), word(ctl, FLAGS)
    cap = int(opts["filter_capacity"])
    count = min(max(word(ctl, COUNT), 0), cap)
    theta_t = float(merit[0])
    phi_t = sigma * float(ft) - mu * float(merit[1])
    dominated = bool(((theta_t >= filt[:count, 0]) & (phi_t >= filt[:count, 1])).any())
    admissible = math.isfinite(phi_t) and math.isfinite(theta_t) and theta_t <= theta_max and not dominated
    switching = False
    if slope < 0.0 and theta0 <= theta_min:
        with np.errstate(all="ignore"):
            lhs = alpha * float(np.power(-slope, opts["s_phi"]))
            rhs = opts["delta"] * float(np.power(theta0, opts["s_theta"]))
        if info is not None:
            info["switching_sides"] = (lhs, rhs)
        switching = lhs > rhs
    armijo = phi_t <= (phi0 + (opts["eta_phi"] * alpha) * slope) + ARMIJO_SLACK * abs(phi0)
    f_theta, f_phi = (1.0 - opts["gamma_theta"]) * theta0, phi0 - opts["gamma_phi"] * theta0
    sufficient = theta_t <= f_theta or phi_t <= f_phi
    ctl[PHI_T], ctl[THETA_T] = phi_t, theta_t
    if admissible and switching and armijo:
        set_word(ctl, STATUS, F_TYPE)
        return ctl, filt, alpha
    if not (admissible and not switching and sufficient):
        half = 0.5 * alpha
        failed = trials + 1 == opts["max_trials"] or half < opts["alpha_floor"]
        set_word(ctl, TRIALS, trials + 1)
        ctl[ALPHA] = 0.0 if failed else half
        if failed:
            set_word(ctl, STATUS, FAILED)
        return ctl, filt, 0.0
    keep = ~((filt[:count, 0] >= f_theta) & (filt[:count, 1] >= f_phi))
    kept = int(keep.sum())
    filt[:kept] = filt[:count][keep]
    if kept < cap:
        filt[kept] = (f_theta, f_phi)
        set_word(ctl, COUNT, kept + 1)
    else:
        set_word(ctl, COUNT, kept)
        set_word(ctl, FLAGS, flags | 2)
    set_word(ctl, STATUS, H_TYPE)
    return ctl, filt, alpha


# ---- the hand-built cases: one per branch of search_accept -------------------------------------------------------------------------
def _filter(entries, cap):
    f = np.full((cap, 2), NAN)
    if len(entries):
        f[:len(entries)] = np.asarray(entries, dtype=np.float64)
    return f


def _far(n, seed):
    """n filter entries that neither block the cases' trial points nor are dominated by their new entries (theta, phi: 50–60, −1000)"""
    rng = np.random.default_rng(seed)
    return [(float(t), -1000.0 - float(p)) for t, p in zip(rng.uniform(50.0, 60.0, n), rng.uniform(0.0, 1.0, n))]


def cases(cap=64):
    """``[(name, control block, filter, ft, merit, mu, sigma, opts, what)]`` with `what` the expected (status, count change kind):
    every branch of search_accept.  mu = 0.1, sigma = 1: phi_t = ft − 0.1·merit[1]."""
    o = dict(OPTS, filter_capacity=cap)
    mu, sg = 0.1, 1.0
    # f-type ground: theta0 = 1e-6 <= theta_min = 1e-4, slope = −2: alpha·2^2.3 = 4.92 > 1·(1e-6)^1.1 = 2.5e-7
    fb = dict(alpha=1.0, alpha_max=1.0, phi0=10.0, theta0=1e-6, slope=-2.0, theta_min=1e-4, theta_max=1e4, phi_t=NAN, theta_t=NAN, status=SEARCHING, flags=1)
    # h-type ground: theta0 = 2.0 > theta_min
    hb = dict(fb, theta0=2.0, slope=-2.0)
    C = []
    add = lambda name, b, f, ft, m, opts=o, **kw: C.append((name, block(**b), _filter(f, opts["filter_capacity"]), ft, np.array(m, dtype=np.float64), mu, sg, opts, kw))
    add("f-type accepted", fb, [], 9.0, [1e-7, 0.0], status=F_TYPE, switching=True)
    add("f-type failing Armijo", fb, [], 10.5, [1e-8, 0.0], status=SEARCHING, switching=True)
    add("h-type accepted by theta", hb, [], 11.0, [1.0, 0.0], status=H_TYPE, switching=False)
    add("h-type accepted by phi", hb, [], 9.0, [3.0, 0.0], status=H_TYPE, switching=False)
    add("h-type rejected", hb, [], 10.5, [2.5, 0.0], status=SEARCHING, switching=False)
    add("dominated by a filter entry", dict(hb, count=3), [(50.0, -1000.0), (0.5, 8.0), (55.0, -1001.0)], 9.0, [1.0, 0.0], status=SEARCHING)
    add("theta_t > theta_max", hb, [], 9.0, [2e4, 0.0], status=SEARCHING)
    add("NaN phi_t", hb, [], NAN, [1.0, 0.0], status=SEARCHING)
    add("inf theta_t", hb, [], 9.0, [float("inf"), 0.0], status=SEARCHING)
    add("max_trials reached", dict(hb, trials=29), [], 10.5, [2.5, 0.0], status=FAILED)
    add("alpha below the floor", dict(hb, alpha=1.5e-16), [], 10.5, [2.5, 0.0], status=FAILED)
    add("already accepted", dict(hb, status=H_TYPE, alpha=0.25, phi_t=9.0, theta_t=1.0), [], 10.5, [2.5, 0.0], status=H_TYPE)
    add("already failed", dict(hb, status=FAILED, alpha=0.0, trials=30), [], 9.0, [1.0, 0.0], status=FAILED)
    add("UNUSABLE", dict(hb, status=UNUSABLE, alpha=0.0, alpha_max=0.0), [], 9.0, [1.0, 0.0], status=UNUSABLE)
    add("filter append", dict(hb, count=2), _far(2, 1), 9.0, [1.0, 0.0], status=H_TYPE, count=3)
    # the new entry is (2·(1 − 1e-5), 10 − 2e-8): entries 1, 3, 4 of six are dominated by it, the other three keep their order
    mixed = [(50.0, -1000.0), (3.0, 11.0), (51.0, -1001.0), (2.5, 10.5), (1e3, 1e3), (52.0, -1002.0)]
    add("dominated entries removed with order kept", dict(hb, count=6), mixed, 9.0, [1.0, 0.0], status=H_TYPE, count=4)
    add("filter full", dict(hb, count=cap), _far(cap, 2), 9.0, [1.0, 0.0], status=H_TYPE, count=cap, overflow=True)
    # the switching condition decides between f-type and h-type: the same trial point, theta0 at and above theta_min
    add("f-type ground, not switching (slope tiny): h-type by theta", dict(fb, slope=-1e-9), [], 9.0, [1e-7, 0.0], status=H_TYPE, switching=False, count=1)
    return C


def filter_sizes(cap):
    """the filter fillings of the GPU test: empty, one, across one wave of 64, and full — as far as the capacity goes"""
    return sorted({k for k in (0, 1, 63, 64, 65, cap) if k <= cap})


def sized_case(count, cap):
    """an h-type acceptance on a filter of `count` entries of which every third is dominated by the new entry; and, with `count`
    even, the trial point is dominated by the LAST entry instead (a rejection that only the last lane of the scan sees)"""
    o = dict(OPTS, filter_capacity=cap)
    far = _far(count, 3 + count)
    ent = [(3.0 + k, 11.0 + k) if k % 3 == 1 else far[k] for k in range(count)]
    b = dict(alpha=0.5, alpha_max=1.0, phi0=10.0, theta0=2.0, slope=-2.0, theta_min=1e-4, theta_max=1e4, phi_t=NAN, theta_t=NAN, status=SEARCHING, flags=1, count=count)
    out = [(f"{count} entries: h-type, every third leaves", block(**b), _filter(ent, cap), 9.0, np.array([1.0, 0.0]), 0.1, 1.0, o, {})]
    if count:
        ent2 = list(far)
        ent2[-1] = (0.5, 8.0)
        out.append((f"{count} entries: dominated by the last", block(**b), _filter(ent2, cap), 9.0, np.array([1.0, 0.0]), 0.1, 1.0, o, {}))
    return out
