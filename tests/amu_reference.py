"""numpy restatement of csrc/iem_amu_device.h — the four words of amu_probe and amu_update blocks in, blocks out, expression for
expression (numpy rounds every operation and contracts nothing: what -ffp-contract=off makes of the kernels) — on top of
tests/mu_reference.py and tests/barrier_reference.py.  TEST INFRASTRUCTURE: tests/test_amu.py (CPU), tests/test_gpu_amu.py,
tests/amu_loop.py.

Two blocks of sixteen float64 words: the iem_mu block (mu_reference) and the object's own — words 0, 2, 11, 12, 13 hold int64 bit
patterns (``mref.ints(blk)`` is the int64 view)."""
import numpy as np

import barrier_reference as bref
import mu_reference as mref

FREE, FIXED = 0, 1
PROBING, LOQO = 0, 1
OPTS = dict(oracle=PROBING, sigma_max=100.0, mu_min=1e-11, mu_max_fact=1e3, init_factor=0.8, red_fact=0.9999, refs_max=4)
F = np.float64
ints = mref.ints
# the own block's words
MODE, MU_MAX, NREFS, REF0, MU_ORACLE, SIGMA, AVG, M_AFF, TO_FIXED, TO_FREE, ORACLE = 0, 1, 2, 3, 7, 8, 9, 10, 11, 12, 13


def options(**over):
    return {**OPTS, **over}


def fresh_block(aopts):
    """the own block behind iem_amu_create / iem_amu_reset: zero but for the oracle's word"""
    blk = np.zeros(16)
    ints(blk)[ORACLE] = aopts["oracle"]
    return blk


def own_block(aopts, mode=FREE, mu_max=0.0, refs=(), to_fixed=0, to_free=0):
    blk = fresh_block(aopts)
    iw = ints(blk)
    iw[MODE], iw[NREFS], iw[TO_FIXED], iw[TO_FREE] = mode, len(refs), to_fixed, to_free
    blk[MU_MAX] = mu_max
    blk[REF0:REF0 + len(refs)] = refs
    return blk


def probe_terms(B, st, sol, dirs, alpha):
    """the products of amu_probe over the present bounds, each operation rounded once (the order: xL, xU, sL, sU — the count and a
    bound on the sum do not depend on it)"""
    x, s, y, zL, zU, vL, vU = st
    ds, dzL, dzU, dvL, dvU = dirs
    ap, ad = F(alpha[0]), F(alpha[1])
    dx = np.asarray(sol)[:len(x)]
    with np.errstate(all="ignore"):
        tx, ts = ap * dx, ap * ds
        return np.concatenate([(((x - B["xl"]) + tx) * (zL + ad * dzL))[B["hasL"]], (((B["xu"] - x) - tx) * (zU + ad * dzU))[B["hasU"]],
                               (((s - B["rl"]) + ts) * (vL + ad * dvL))[B["gL"]], (((B["ru"] - s) - ts) * (vU + ad * dvU))[B["gU"]]])


def probe_words(B, st, sol, dirs, alpha):
    """``(terms of word 0, word 1, word 2, word 3)``"""
    p = probe_terms(B, st, sol, dirs, alpha)
    return p, float(np.isnan(p).sum()), float(alpha[0]), float(alpha[1])


def probe_addends(B, st, sol, dirs, alpha):
    """the products of amu_probe over [0, nvar + ncon) in the kernel's statement order: ``(pL, pU)`` — lower then upper on a variable
    and on an inequality row, +0.0 where the bound is absent"""
    x, s, y, zL, zU, vL, vU = st
    ds, dzL, dzU, dvL, dvU = dirs
    ap, ad = F(alpha[0]), F(alpha[1])
    dx = np.asarray(sol)[:len(x)]
    with np.errstate(all="ignore"):
        tx, ts = ap * dx, ap * ds
        pL = bref.full(B, B["hasL"], ((x - B["xl"]) + tx) * (zL + ad * dzL), B["gL"], ((s - B["rl"]) + ts) * (vL + ad * dvL))
        pU = bref.full(B, B["hasU"], ((B["xu"] - x) - tx) * (zU + ad * dzU), B["gU"], ((B["ru"] - s) - ts) * (vU + ad * dvU))
    return pL, pU


def probe_sum(B, st, sol, dirs, alpha, n_wg):
    """word 0 of amu_probe on a grid of `n_wg` workgroups: the device's bits"""
    return bref.device_sum(list(probe_addends(B, st, sol, dirs, alpha)), n_wg)


def directions(P, seed=7):
    """a random sol = [dx; dy] and, from it, barrier_reference.step at tau = 1: ``(sol, dirs, alpha)`` on the host — NaN on equality rows"""
    B, st = P["B"], P["state"]
    n, m = len(st[0]), len(st[1])
    rng = np.random.default_rng(seed)
    sol = 0.1 * rng.standard_normal(n + m)
    dirs, alpha = bref.step(B, st, sol, tuple(np.full(m, np.nan) for _ in range(3)), bref.MU, 1.0)
    return sol, dirs, alpha


def _ring(ab):
    return int(min(max(ints(ab)[NREFS], 0), 4))


def _remember(ab, refs_max, e0):
    n = _ring(ab)
    if n >= refs_max:
        ab[REF0:REF0 + n - 1] = ab[REF0 + 1:REF0 + n].copy()
        n -= 1
    ab[REF0 + n] = e0
    ints(ab)[NREFS] = n + 1


def _is_plus_zero(v):
    return F(v).view(np.int64) == 0


def update(blk, ab, w, probe, counts, opts, aopts, force_fixed=False, ctl=None):
    """amu_update: ``(mu block, own block, ctl)`` after the call — ``probe`` the four words or None (LOQO), ``ctl`` a search's control
    block (16 words) or None"""
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
    probing = aopts["oracle"] == PROBING
    k = 0
    unusable = w[10] != 0.0 or np.isnan(e0)
    if probing:
        q = np.asarray(probe, dtype=np.float64)
        unusable = unusable or q[1] != 0.0 or _is_plus_zero(q[2]) or _is_plus_zero(q[3])
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
            ab[AVG] = avg
            mu_hi = F(ab[MU_MAX])
            if _is_plus_zero(mu_hi):
                mu_hi = F(aopts["mu_max_fact"]) * avg
                ab[MU_MAX] = mu_hi
            nref = _ring(ab)
            progress = nref < aopts["refs_max"]
            if not progress:
                worst = F(ab[REF0])
                for i in range(1, nref):
                    worst = np.maximum(worst, ab[REF0 + i])
                progress = bool(e0 <= F(aopts["red_fact"]) * worst)
            mode = int(ia[MODE])
            if mode == FIXED:
                if progress:
                    mode = FREE
                    ia[TO_FREE] += 1
                    _remember(ab, aopts["refs_max"], e0)
                else:
                    while mu > floor and Emu(mu) <= kappa_eps * mu and k < mref.MAX_DECREASES:
                        mu = np.maximum(floor, np.minimum(kappa_mu * mu, mu * np.sqrt(mu)))
                        k += 1
            else:
                if progress and not force_fixed:
                    _remember(ab, aopts["refs_max"], e0)
                else:
                    mode = FIXED
                    ia[TO_FIXED] += 1
                    mu = np.minimum(np.maximum(F(aopts["init_factor"]) * avg, mu_min), mu_hi)
            ia[MODE] = mode
            if mode == FREE:
                m_aff = F(0.0)
                if probing:
                    m_aff = q[0] / F(nz)
                    r = m_aff / avg
                    sigma = np.minimum((r * r) * r, F(aopts["sigma_max"]))
                else:
                    xi = w[8] / avg
                    f = (F(0.05) * (F(1.0) - xi)) / xi
                    c = np.minimum(f, F(2.0))
                    sigma = F(0.1) * ((c * c) * c)
                mu_or = sigma * avg
                ab[MU_ORACLE], ab[SIGMA], ab[M_AFF] = mu_or, sigma, m_aff
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


def words(nz, d=1e-3, p=0.0, pmax=2e-2, pmin=5e-3, avg=1e-2, bad=0.0):
    """twelve hand-made words: the sums 4 and 5 are 1, so sd = sc = 1 and  E(mu) = max(d, p, max(pmax − mu, mu − pmin));  word 9 is
    avg·nz"""
    w = np.zeros(12)
    w[0] = w[1] = d
    w[2], w[3], w[8] = p, pmax, pmin
    w[4] = w[5] = 1.0
    w[9] = avg * max(nz, 0)
    w[10] = bad
    return w


def branch_cases(oracle, counts):
    """Hand-made inputs that reach every branch of amu_update for a model with ``counts = (ncon, nz)``:
    ``dict(label, w, probe, blk, ab, opts, aopts, force_fixed, want)`` — ``want`` holds what the branch is known by (a subset of
    status, mode, k, changed, nrefs, mu, sigma, to_fixed, to_free), checked against the restatement in tests/test_amu.py.  With
    ``nz = 0`` only the branches that a model without bounds can reach."""
    m, nz = int(counts[0]), int(counts[1])
    opts = mref.options()
    ao = options(oracle=oracle)
    probing = oracle == PROBING
    avg = 1e-2
    out = []

    def probe(ratio=0.5, bad=0.0, ap=0.75, ad=0.5):
        return np.array([ratio * avg * nz, bad, ap, ad]) if probing else None

    def case(label, w, q=None, mu0=0.1, ab=None, o=opts, a=ao, force=False, flags=0, **want):
        blk = mref.fresh_block(o, mu0)
        ints(blk)[9] = flags
        out.append(dict(label=label, w=w, probe=q if q is not None else probe(), blk=blk, ab=fresh_block(a) if ab is None else ab, opts=o, aopts=a,
                        force_fixed=force, want=want))

    W = lambda **kw: words(nz, **kw)
    full = lambda v: (v,) * 4
    case("unusable: a product did not enter", W(bad=1.0), flags=1, status=mref.UNUSABLE, changed=False, nrefs=0)
    case("unusable: E(0) is a NaN", W(d=np.nan), status=mref.UNUSABLE, changed=False)
    case("converged", W(d=1e-10, pmax=1e-10, pmin=1e-10, avg=1e-10), flags=1, status=mref.CONVERGED, changed=False, nrefs=0)
    if nz == 0:
        case("nz = 0: mu_min", W(), status=mref.ITERATING, changed=True, mu=ao["mu_min"], mode=FREE, nrefs=0)
        case("nz = 0: mu stays", W(), mu0=ao["mu_min"], flags=1, status=mref.ITERATING, changed=False, mode=FREE)
        return out
    if probing:
        case("unusable: a NaN product in the probe", W(), probe(bad=1.0), status=mref.UNUSABLE, changed=False)
        case("unusable: alpha_p is +0.0", W(), probe(ap=0.0), status=mref.UNUSABLE, changed=False)
        case("unusable: alpha_d is +0.0", W(), probe(ad=0.0), status=mref.UNUSABLE, changed=False)
    set_max = 1e3 * avg
    case("the first update sets mu_max", W(), status=mref.ITERATING, mode=FREE, nrefs=1, changed=True, mu_max=F(1e3) * F(avg))
    case("free, progress, the ring filling", W(), ab=own_block(ao, FREE, set_max, (1.0, 0.5)), mode=FREE, nrefs=3, to_fixed=0)
    case("free, progress, a full ring: the oldest leaves", W(), ab=own_block(ao, FREE, set_max, (1.0, 0.5, 0.3, 0.1)), mode=FREE, nrefs=4, refs_head=0.5)
    case("free to fixed: no progress", W(), ab=own_block(ao, FREE, set_max, full(1e-3)), mode=FIXED, to_fixed=1, nrefs=4, changed=True,
         mu=np.minimum(np.maximum(F(0.8) * F(avg), F(1e-11)), F(set_max)))
    case("free to fixed: forced", W(), ab=own_block(ao, FREE, set_max, (1.0,)), force=True, mode=FIXED, to_fixed=1, nrefs=1)
    case("fixed, no decrease: mu unchanged", W(), mu0=1e-4, ab=own_block(ao, FIXED, set_max, full(1e-3), to_fixed=1), flags=1, mode=FIXED, k=0, changed=False)
    one = mref.options(kappa_eps=1.0, kappa_mu=1e-6)
    case("fixed, one decrease", W(), ab=own_block(ao, FIXED, set_max, full(1e-3), to_fixed=1), o=one, mode=FIXED, k=1, changed=True)
    case("fixed, several decreases", W(), ab=own_block(ao, FIXED, set_max, full(1e-3), to_fixed=1), mode=FIXED, k=3, changed=True)
    case("fixed to free", W(), ab=own_block(ao, FIXED, set_max, full(1.0), to_fixed=1), mode=FREE, to_free=1, nrefs=4, k=0)
    short = options(oracle=oracle, refs_max=2)
    case("a ring of two", W(), ab=own_block(short, FREE, set_max, (1.0, 0.5)), a=short, mode=FREE, nrefs=2, refs_head=0.5)
    if probing:
        case("probing: unclamped", W(), probe(0.5), ab=own_block(ao, FREE, set_max), sigma=0.125, mu=F(0.125) * F(avg))
        case("probing: clamped at mu_min", W(), probe(1e-5), ab=own_block(ao, FREE, set_max), mu=ao["mu_min"])
        case("probing: clamped at mu_max", W(), probe(2.0), ab=own_block(ao, FREE, 2.0 * avg), sigma=8.0, mu=2.0 * avg)
        case("probing: sigma capped by sigma_max", W(), probe(10.0), ab=own_block(ao, FREE, set_max), sigma=100.0, mu=F(100.0) * F(avg))
    else:
        case("LOQO: unclamped, xi = 1/2", W(pmin=0.5 * avg), ab=own_block(ao, FREE, set_max), sigma=F(0.1) * ((F(0.05) * F(0.05)) * F(0.05)))
        case("LOQO: xi = 1, clamped at mu_min", W(pmax=avg, pmin=avg), ab=own_block(ao, FREE, set_max), sigma=0.0, mu=ao["mu_min"])
        case("LOQO: xi = 0", W(pmin=0.0), ab=own_block(ao, FREE, set_max), sigma=F(0.1) * F(8.0), mu=(F(0.1) * F(8.0)) * F(avg))
        case("LOQO: xi = 0, clamped at mu_max", W(pmin=0.0), ab=own_block(ao, FREE, 0.5 * avg), sigma=F(0.1) * F(8.0), mu=0.5 * avg)
    # the oracle lands on the mu the block holds: nothing changed, the flag is cleared, the filter stays
    last = out[-4]
    again, _, _ = update(last["blk"], last["ab"], last["w"], last["probe"], counts, last["opts"], last["aopts"])
    case("free: the oracle's mu is the block's", last["w"], last["probe"], mu0=float(again[0]), ab=last["ab"], flags=1, mode=FREE, changed=False)
    return out
