"""numpy restatement of csrc/iem_conv_device.h — conv_xmax / conv_decide, conv_stepmax / conv_step_decide, conv_keep, conv_restore —
block in, block out, one rounded operation per line (numpy rounds every operation and contracts nothing: what -ffp-contract=off makes
of the kernels), on top of tests/barrier_reference.py and tests/mu_reference.py.  TEST INFRASTRUCTURE: tests/test_conv.py (CPU),
tests/test_gpu_conv.py, tests/conv_loop.py.

The block is a float64 array of twenty-four words; words 0–7 hold int64 bit patterns (``ints(blk)`` is the int64 view).  Vectors are
full length; where the kernels branch on a presence flag the restatement selects with np.where: the selected entries carry the same
bits.  Entries of s, vL, vU on equality rows pass through untouched."""
import numpy as np

import mu_reference as mref

STATUS, CHECKS, ACC_COUNT, KEEP, KEPT, KEPT_AT, FLAGS, TINY_COUNT, E0, D, P, CPL, F_, F_PREV, XMAX, KEPT_E0, KEPT_F, REL, DYMAX = range(19)
WORDS = 24
ITERATING, CONVERGED, ACCEPTABLE, MAXITER, DIVERGING, INVALID, TINY_STEP = range(7)
OPTS = dict(dual_inf_tol=1.0, constr_viol_tol=1e-4, compl_inf_tol=1e-4, acceptable_tol=1e-6, acceptable_iter=15, acceptable_dual_inf_tol=1e10,
            acceptable_constr_viol_tol=1e-2, acceptable_compl_inf_tol=1e-2, acceptable_obj_change_tol=1e20, max_iter=3000, diverging_iterates_tol=1e20,
            tiny_step_tol=10.0 * 2.0 ** -52, tiny_step_y_tol=1e-2)
F = np.float64


def options(**over):
    unknown = set(over) - set(OPTS)
    assert not unknown, unknown
    return {**OPTS, **over}


def ints(blk):
    return blk.view(np.int64)


def fresh_block():
    """the block behind iem_conv_create / iem_conv_reset"""
    return np.zeros(WORDS)


def fresh_kept(nvar, ncon):
    """the kept buffers behind iem_conv_create: (x, s, y, zL, zU, vL, vU), zero"""
    return tuple(np.zeros(k) for k in (nvar, ncon, ncon, nvar, nvar, ncon, ncon))


# ---- the integer maxima on bit patterns ---------------------------------------------------------------------------------------------------
def bits_max(values):
    """the maximum of the bit patterns of |values| from the seed +0.0, as a double: order-independent, a NaN beats every number"""
    v = np.ascontiguousarray(values, dtype=np.float64)
    top = np.abs(v).view(np.uint64).max() if len(v) else np.uint64(0)
    return np.array([top], dtype=np.uint64).view(np.float64)[0]


def xmax(x):
    """conv_xmax"""
    return bits_max(x)


def stepmax(B, x, s, sol, ds):
    """conv_stepmax: ``(rel, dymax)``; s and ds on equality rows are not read"""
    nvar = len(x)
    with np.errstate(all="ignore"):
        den_x = F(1.0) + np.abs(x)
        q_x = np.abs(sol[:nvar]) / den_x
        ine = ~B["eq"]
        den_s = F(1.0) + np.abs(s[ine])
        q_s = np.abs(ds[ine]) / den_s
    return bits_max(np.concatenate([q_x, q_s])), bits_max(sol[nvar:])


# ---- conv_decide --------------------------------------------------------------------------------------------------------------------------
def e0_terms(w, counts, mu_opts):
    """``(E(0), d, p, cpl)`` from the twelve words: E(0) in mu_reference's expressions at mu = +0.0"""
    w = np.asarray(w, dtype=np.float64)
    m, nz = int(counts[0]), int(counts[1])
    e_d, e_p, sc = mref.terms(w, counts, mu_opts)
    ec0 = mref.e_c(w, counts, sc, F(0.0))
    with np.errstate(all="ignore"):
        e0 = np.maximum(np.maximum(e_d, e_p), ec0)
        d = np.maximum(w[0], w[1])
    p = w[2] if m else F(0.0)
    cpl = w[3] if nz else F(0.0)
    return F(e0), F(d), F(p), F(cpl)


def decide(blk, w, f, x_max, counts, opts, mu_opts):
    """conv_decide: the block after iem_conv_check — w the twelve words, f the objective, x_max the slot; mu_opts the RESOLVED options
    of the iem_mu object (mu_reference.options): tol and s_max"""
    blk = blk.copy()
    iw = ints(blk)
    if iw[STATUS] != ITERATING:      # latched: keep = 0 and nothing else
        iw[KEEP] = 0
        return blk
    w = np.asarray(w, dtype=np.float64)
    f, x_max = F(f), F(x_max)
    e0, d, p, cpl = e0_terms(w, counts, mu_opts)
    checks = int(iw[CHECKS])
    f_prev = F(blk[F_])
    count, kept, kept_at = int(iw[ACC_COUNT]), int(iw[KEPT]), int(iw[KEPT_AT])
    kept_e0, kept_f = F(blk[KEPT_E0]), F(blk[KEPT_F])
    status, keep, acceptable = ITERATING, 0, 0
    o = {k: (F(v) if isinstance(v, float) else v) for k, v in opts.items()}
    with np.errstate(all="ignore"):
        if w[10] != 0.0 or np.isnan(e0) or np.isnan(f) or np.isnan(x_max) or np.isinf(e0) or np.isinf(f):
            status = INVALID
        elif e0 <= F(mu_opts["tol"]) and d <= o["dual_inf_tol"] and p <= o["constr_viol_tol"] and cpl <= o["compl_inf_tol"]:
            status, keep = CONVERGED, 1
        else:
            small_change = checks == 0
            if not small_change:
                diff = np.abs(f - f_prev)
                den = np.maximum(F(1.0), np.abs(f))
                small_change = bool(diff / den <= o["acceptable_obj_change_tol"])
            acc = bool(e0 <= o["acceptable_tol"] and d <= o["acceptable_dual_inf_tol"] and p <= o["acceptable_constr_viol_tol"] and
                       cpl <= o["acceptable_compl_inf_tol"] and small_change)
            acceptable = int(acc)
            count = count + 1 if acc else 0
            if acc and (kept == 0 or e0 <= kept_e0):
                keep = 1
            if o["acceptable_iter"] > 0 and count >= o["acceptable_iter"]:
                status = ACCEPTABLE
            elif checks >= o["max_iter"]:
                status = MAXITER
            elif x_max > o["diverging_iterates_tol"]:
                status = DIVERGING
    if keep:
        kept, kept_at, kept_e0, kept_f = 1, checks, e0, f
    iw[STATUS] = status
    iw[CHECKS] = checks + 1 if status == ITERATING else checks
    iw[ACC_COUNT] = count
    iw[KEEP] = keep
    iw[KEPT] = kept
    iw[KEPT_AT] = kept_at
    iw[FLAGS] = (int(iw[FLAGS]) & ~1) | acceptable
    blk[E0], blk[D], blk[P], blk[CPL], blk[F_], blk[F_PREV], blk[XMAX], blk[KEPT_E0], blk[KEPT_F] = e0, d, p, cpl, f, f_prev, x_max, kept_e0, kept_f
    return blk


def check(blk, w, f, x, counts, opts, mu_opts):
    """iem_conv_check: conv_xmax, then conv_decide"""
    return decide(blk, w, f, xmax(x), counts, opts, mu_opts)


# ---- conv_step_decide ---------------------------------------------------------------------------------------------------------------------
def step_decide(blk, rel, dymax, mu, opts, mu_opts):
    """conv_step_decide: the block after iem_conv_step — rel, dymax the slots, mu word 0 of the iem_mu block"""
    blk = blk.copy()
    iw = ints(blk)
    if iw[STATUS] != ITERATING:      # latched: nothing
        return blk
    rel, dymax, mu = F(rel), F(dymax), F(mu)
    floor = F(mu_opts["mu_floor"])
    with np.errstate(invalid="ignore"):
        tiny = bool(rel < F(opts["tiny_step_tol"]))      # a NaN compares false
        count = int(iw[TINY_COUNT]) + 1 if tiny else 0
        at_floor = bool(mu <= floor)
        flags = int(iw[FLAGS]) & 1
        if tiny:
            flags |= 2
        if tiny and bool(mu > floor):
            flags |= 4
        if count >= 2 and bool(dymax < F(opts["tiny_step_y_tol"])) and at_floor:
            iw[STATUS] = TINY_STEP
    iw[FLAGS] = flags
    iw[TINY_COUNT] = count
    blk[REL], blk[DYMAX] = rel, dymax
    return blk


def step(blk, B, x, s, sol, ds, mu, opts, mu_opts):
    """iem_conv_step: conv_stepmax, then conv_step_decide"""
    rel, dymax = stepmax(B, x, s, sol, ds)
    return step_decide(blk, rel, dymax, mu, opts, mu_opts)


# ---- conv_keep, conv_restore --------------------------------------------------------------------------------------------------------------
def keep(blk, B, st, held):
    """iem_conv_keep: the kept buffers after the call — on the word keep; +0.0 where a bound is absent, equality rows of s, vL, vU as
    they were"""
    if ints(blk)[KEEP] == 0:
        return tuple(a.copy() for a in held)
    x, s, y, zL, zU, vL, vU = st
    ine = ~B["eq"]
    return (x.copy(), np.where(ine, s, held[1]), y.copy(), np.where(B["hasL"], zL, 0.0), np.where(B["hasU"], zU, 0.0),
            np.where(ine, np.where(B["gL"], vL, 0.0), held[5]), np.where(ine, np.where(B["gU"], vU, 0.0), held[6]))


def restore(blk, B, held, st):
    """iem_conv_restore: the state after the call — on the word kept; only the entries keep reads are written"""
    if ints(blk)[KEPT] == 0:
        return tuple(a.copy() for a in st)
    x, s, y, zL, zU, vL, vU = st
    ine = ~B["eq"]
    return (held[0].copy(), np.where(ine, held[1], s), held[2].copy(), np.where(B["hasL"], held[3], zL), np.where(B["hasU"], held[4], zU),
            np.where(ine & B["gL"], held[5], vL), np.where(ine & B["gU"], held[6], vU))
