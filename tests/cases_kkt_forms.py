"""One list of chain KKT kernel FORMS (csrc/iem_kkt_device.h, csrc/iem_kkt_many_device.h): a shape (nb, ne, nc) per code path
that the shapes of the named models never reach, synthetic well-conditioned blocks for each, and a dense reference.

Read by build() (the 15 code objects are precompiled: no test compiles one), by tests/test_kkt_forms.py (CPU: the generator's
conditions, the dispatch witness, the admission sweep) and by tests/test_gpu_kkt_forms.py (the kernels against the reference).

`defs` of a form: what the head of kkt_source(nb, ne, nc) must define for the row to be a witness of its path — rowwise =
KKT_ROWWISE (rows per lane; 0: the MFMA panel form), wpg = KKT_ROW_WPG, wmax = KKT_WMAX (the header's default 4 when absent),
wpe = KKT_WPE (0 when absent: the compiler's choice), mr = KKT_MR (columns per chunk of the multi-column solves).  What follows
from them, as csrc/iem_kkt_device.h derives it: `lanes` = (blocks per workgroup, idle lanes) and `lane_solves` (kkt_fz / kkt_fs /
kkt_bw instead of the 64-thread solves) of a lane-per-row form; `tiles` = (tile rows R, waves W, a partial last tile row in
some wave, a padded rim) of a panel form; `update_threads` = KKT_TU."""
import functools

import numpy as np

import chain_reference as ref

LDS_BYTES = 160 * 1024

FORMS = [
    # ---- lane-per-row eliminate ---------------------------------------------------------------------------------------------
    dict(shape=(4, 0, 4), lanes=(32, 0), lane_solves=True, update_threads=64, defs=dict(rowwise=2, wpg=1, wmax=4, wpe=4, mr=4), extra_S=131,
         path="smallest admitted; 2 rows/lane, 32 blocks per wave, 16 blocks per solve wave"),
    dict(shape=(12, 0, 4), lanes=(21, 2), lane_solves=True, update_threads=64, defs=dict(rowwise=2, wpg=2, wmax=4, wpe=4, mr=4), extra_S=131,
         path="2 rows/lane and 2-wave workgroup, 21 blocks + 2 shadow lanes"),
    dict(shape=(24, 0, 20), lanes=(5, 4), lane_solves=True, update_threads=256, defs=dict(rowwise=2, wpg=1, wmax=4, wpe=4, mr=2), extra_S=67,
         path="2 rows/lane, 5 blocks + 4 idle lanes; KKT_MR 2; kkt_update at 256 threads"),
    dict(shape=(28, 0, 8), lanes=(2, 8), lane_solves=True, update_threads=64, defs=dict(rowwise=1, wpg=1, wmax=4, wpe=4, mr=4), extra_S=67,
         path="1 row/lane with lane-per-row solves, 8 idle lanes; kkt_update at 64 threads"),
    dict(shape=(32, 0, 32), lanes=(2, 0), lane_solves=True, update_threads=256, defs=dict(rowwise=1, wpg=1, wmax=4, wpe=4, mr=2), extra_S=67,
         path="1 row/lane, full wave; nc = nb; KKT_MR 2"),
    dict(shape=(36, 0, 12), lanes=(3, 20), lane_solves=False, update_threads=128, defs=dict(rowwise=1, wpg=2, wmax=1, wpe=3, mr=4), extra_S=67,
         path="1 row/lane, 2-wave workgroup (3 blocks on 128 lanes), 64-thread solves"),
    # ---- panel form, no border ----------------------------------------------------------------------------------------------
    dict(shape=(48, 0, 48), tiles=(3, 1, False, False), update_threads=256, defs=dict(rowwise=0, wpg=0, wmax=1, wpe=3, mr=4), path="R = 3, no rim, one wave; largest nc"),
    dict(shape=(64, 0, 16), tiles=(4, 2, False, False), update_threads=128, defs=dict(rowwise=0, wpg=0, wmax=2, wpe=3, mr=4), path="R = 4, no rim"),
    dict(shape=(72, 0, 12), tiles=(5, 2, True, True), update_threads=128, defs=dict(rowwise=0, wpg=0, wmax=2, wpe=2, mr=4), path="R = 5: two waves, partial last tile row"),
    dict(shape=(96, 0, 24), tiles=(6, 2, False, False), update_threads=256, defs=dict(rowwise=0, wpg=0, wmax=2, wpe=2, mr=4), path="R = 6, no rim, as a chain (not the ne = -1 leaf)"),
    # ---- panel form, bordered -----------------------------------------------------------------------------------------------
    dict(shape=(16, 16, 8), tiles=(1, 1, False, False), update_threads=64, defs=dict(rowwise=0, wpg=0, wmax=4, wpe=4, mr=4), path="one tile each way, no rim, one wave"),
    dict(shape=(36, 8, 12), tiles=(3, 3, False, True), update_threads=128, defs=dict(rowwise=0, wpg=0, wmax=4, wpe=4, mr=4),
         path="a lane-per-row size pushed to the panel form by its border; W = 3"),
    dict(shape=(72, 20, 8), tiles=(5, 4, True, True), update_threads=64, defs=dict(rowwise=0, wpg=0, wmax=4, wpe=0, mr=4),
         path="R = 5 under four waves (partial tile rows in waves 1..3), border rim"),
    dict(shape=(84, 64, 4), tiles=(6, 4, True, True), update_threads=64, defs=dict(rowwise=0, wpg=0, wmax=4, wpe=0, mr=4),
         path="largest border that fits the LDS at nb = 84 (158 888 bytes), RE = 4 exact"),
    dict(shape=(20, 128, 4), tiles=(2, 2, False, True), update_threads=64, defs=dict(rowwise=0, wpg=0, wmax=4, wpe=4, mr=4), path="largest ne"),
]
SHAPES = [f["shape"] for f in FORMS]


def declared_lds(nb, ne, defs=None):
    """Bytes of LDS kkt_eliminate DECLARES for a shape, restated from csrc/iem_kkt_device.h.  Lane-per-row form (`defs` of the
    form, or the host's rule restated: no border, two rows per lane up to 24, one up to 40): rowbuf[2][KKT_BPW * NB] doubles and
    cnt[2] ints.  Panel form: panels[KKT_PANEL_DOUBLES + 2 KKT_GJ_DOUBLES] doubles = 2 16R 5 + 2 4 (16R + 1) + 64 with
    R = ceil(nb / 16), the two int counters, and with a border M[NB (NB + 1)], EE and ZZ[NB (NE + 1)] doubles."""
    rpl = defs["rowwise"] if defs else (0 if ne != 0 or nb > 40 else 2 if nb <= 24 else 1)
    if rpl:
        lpb = nb // rpl
        wpg = defs["wpg"] if defs else (2 if (128 // lpb) * 64 > (64 // lpb) * 128 else 1)
        return 8 * 2 * ((64 * wpg) // lpb) * nb + 8
    R = (nb + 15) // 16
    return 8 * (2 * 16 * R * 5 + 2 * 4 * (16 * R + 1) + 64) + 8 + (8 * nb * (nb + 1) + 16 * nb * (ne + 1) if ne > 0 else 0)


class Case:
    """One (form, variant): `kind` chain / shared / unchained / laned, S blocks (lanes x T when laned)."""

    def __init__(self, shape, kind, S, lanes=1):
        self.shape, self.kind, self.S, self.lanes = shape, kind, S, lanes
        self.T = S // lanes
        self.id = "%d-%d-%d-%s-S%d" % (*shape, kind, S) + ("x%d" % self.T if kind == "laned" else "")
        self.n = S * shape[0] + shape[1]

    def __repr__(self):
        return self.id


def _cases():
    out = []
    for f in FORMS:
        for S in (1, 2, 3, 11) + ((f["extra_S"],) if "extra_S" in f else ()):
            out.append(Case(f["shape"], "chain", S))
    out += [Case((36, 0, 12), "shared", 11), Case((36, 8, 12), "shared", 11)]
    out += [Case((28, 0, 8), "unchained", 5), Case((16, 16, 8), "unchained", 5), Case((72, 20, 8), "unchained", 3)]
    out += [Case((28, 0, 8), "laned", 15, lanes=3), Case((72, 0, 12), "laned", 6, lanes=2), Case((4, 0, 4), "laned", 120, lanes=40)]
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
NRHS_MAX = 5      # KKT_MR + 1 columns at the most


class Data:
    pass


@functools.lru_cache(maxsize=None)
def data(case_id):
    """Blocks of a case (the recipe of the former tools/probes/kkt_block_probe.py): D_k = [[H, J'], [J, -I/2]] with H = A A' / nv + 2 I and
    nv = 5 nb // 9 variables; the coupling rows R among the constraint rows and columns C among the variables, |R| = min(nc - 1,
    nb - nv), |C| = min(max(nc - 2, 1), nv) (fewer than nc: the -1 padding of rows / cols is exercised); Bt = 0.5 N(0, 1),
    E = 0.3 N(0, 1) / sqrt(nb), G = 3 I.  `shared`: one variable index sits in R AND in C, coupling scale 0.05.  `unchained`: no
    coupling at all.  `laned`: no coupling across a seam (the Bt of a lane's first block holds values nobody may read).
    The seed depends on the shape and the variant only."""
    c = BY_ID[case_id]
    nb, ne, nc = c.shape
    S, T = c.S, c.T
    rng = np.random.default_rng([nb, ne, nc, S, ["chain", "shared", "unchained", "laned"].index(c.kind)])
    nv = (nb * 5) // 9
    R = np.sort(rng.choice(np.arange(nv, nb), size=min(nc - 1, nb - nv), replace=False))
    Cc = np.sort(rng.choice(np.arange(nv), size=min(max(nc - 2, 1), nv), replace=False))
    scale = 0.5
    if c.kind == "shared":
        R = np.sort(np.concatenate([R[1:], Cc[:1]]))      # a variable row joins R: R and C share the local index Cc[0]
        scale = 0.05
    d = Data()
    d.case, d.R, d.C = c, R, Cc
    d.D = np.zeros((S, nb, nb))
    d.B = np.zeros((S, nb, nb))
    d.Bt = np.zeros((S, nc, nc))
    d.E = 0.3 * rng.standard_normal((S, nb, ne)) / np.sqrt(nb)
    for k in range(S):
        H = rng.standard_normal((nv, nv))
        H = H @ H.T / nv + 2.0 * np.eye(nv)
        J = rng.standard_normal((nb - nv, nv)) / np.sqrt(nv)
        d.D[k, :nv, :nv] = H
        d.D[k, nv:, :nv] = J
        d.D[k, :nv, nv:] = J.T
        d.D[k, nv:, nv:] = -0.5 * np.eye(nb - nv)
        if k % T and c.kind != "unchained":
            d.Bt[k, :R.size, :Cc.size] = scale * rng.standard_normal((R.size, Cc.size))
            d.B[k][R[:, None], Cc[None, :]] = d.Bt[k, :R.size, :Cc.size]
    d.G = 3.0 * np.eye(ne)
    d.rhs = rng.standard_normal((NRHS_MAX, S, nb))
    d.rB = rng.standard_normal((NRHS_MAX, ne))
    d.rows = np.full(nc, -1, np.int32)
    d.rows[:R.size] = R
    d.cols = np.full(nc, -1, np.int32)
    d.cols[:Cc.size] = Cc
    d.junk = rng.standard_normal((nc, nc))               # what the device's Bt holds where no coupling exists (first block of a lane)
    return d


def dense_K(d):
    """The whole system, blocks in order, the border last: [[blockdiag(D) + B sub-diagonals, E], [E', G]]."""
    c = d.case
    nb, ne, _ = c.shape
    n = c.n
    K = np.zeros((n, n))
    for k in range(c.S):
        K[k * nb:(k + 1) * nb, k * nb:(k + 1) * nb] = d.D[k]
        if k % c.T:
            K[k * nb:(k + 1) * nb, (k - 1) * nb:k * nb] = d.B[k]
            K[(k - 1) * nb:k * nb, k * nb:(k + 1) * nb] = d.B[k].T
        if ne:
            K[k * nb:(k + 1) * nb, c.S * nb:] = d.E[k]
            K[c.S * nb:, k * nb:(k + 1) * nb] = d.E[k].T
    if ne:
        K[c.S * nb:, c.S * nb:] = d.G
    return K


def refined_solve(K, rhs):
    """x_ref: LU in float64, then refinement with the residuals formed in numpy.longdouble, until the correction is below
    1e-17 max |x| (columns of `rhs` are right-hand sides)."""
    import scipy.linalg as sla
    lu = sla.lu_factor(K)
    Kl, bl = K.astype(np.longdouble), rhs.astype(np.longdouble)
    x = sla.lu_solve(lu, rhs).astype(np.longdouble)
    for _ in range(12):
        dx = sla.lu_solve(lu, (bl - Kl @ x).astype(np.float64))
        x = x + dx
        if np.abs(dx).max() <= 1e-17 * np.abs(x).max():
            break
    else:
        raise AssertionError("the refinement of the dense reference did not settle")
    return x.astype(np.float64)


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(b).max())) if np.size(b) else 0.0


class Reference:
    pass


@functools.lru_cache(maxsize=None)
def reference(case_id):
    """Everything a test compares with, computed ONCE per case and process and never written to:
       x_ref (NRHS_MAX, n)    the dense refined solutions, column u for the right-hand side u
       Dinv, Z, Gp, neg       tests/chain_reference.py's factors, every lane a chain of its own
       xs, xB                 its solutions;  err_cols[u] = max |x - x_ref| / max(1, max |x_ref|) of column u, err_cpu = err_cols[0]
       bounds[u]              16 max(err_cols[u], n 2^-52): what the device's column u may differ from x_ref[u] by
       err_inv                (a recorded figure, no bound uses it) the error of the restatement's own float64 inverses: against one Newton-Schulz step X + X (I - M X)
                              in longdouble on the matrices M it inverted
       min_pivot              the smallest |pivot| of its eliminations"""
    d = data(case_id)
    c = d.case
    nb, ne, _ = c.shape
    S, T = c.S, c.T
    r = Reference()
    K = dense_K(d)
    full = np.concatenate([d.rhs.reshape(NRHS_MAX, S * nb), d.rB], axis=1)
    r.x_ref = refined_solve(K, full.T).T.copy()
    r.Dinv, r.Z, r.Gp = np.zeros((S, nb, nb)), np.zeros((S, nb, ne)), np.zeros((S, ne, ne))
    r.X, r.Y = np.zeros((S, nb, nb)), np.zeros((S, nb, nb))
    r.neg, r.min_pivot, r.err_inv = 0, np.inf, 0.0
    pre = {}
    lanes = [slice(k, k + 1) for k in range(S)] if c.kind == "unchained" else [slice(a * T, (a + 1) * T) for a in range(c.lanes)]
    for sl in lanes:
        pre.clear()
        Di, X, Y, Z, Gp, neg = ref.factor(d.D[sl], d.B[sl], d.E[sl], pre=pre)
        r.Dinv[sl], r.X[sl], r.Y[sl], r.Z[sl], r.Gp[sl] = Di, X, Y, Z, Gp
        r.neg += neg
        for i, M in pre.items():
            P = M.copy()
            for k in range(nb):
                r.min_pivot = min(r.min_pivot, abs(P[k, k]))
                P[k + 1:, k + 1:] -= np.outer(P[k + 1:, k], P[k, k + 1:]) / P[k, k]
            Ml, Xl = M.astype(np.longdouble), Di[i].astype(np.longdouble)
            r.err_inv = max(r.err_inv, rel(Di[i], (Xl + Xl @ (np.eye(nb, dtype=np.longdouble) - Ml @ Xl)).astype(np.float64)))
    # the solves: a border couples the lanes of an unchained case through x_B, so the border system is formed over all of them
    r.xs, r.xB = np.zeros((NRHS_MAX, S, nb)), np.zeros((NRHS_MAX, ne))
    for u in range(NRHS_MAX):
        if c.kind == "unchained":
            rBp = np.einsum("kbe,kb->ke", r.Z, d.rhs[u])
            xB = np.linalg.solve(d.G - r.Gp.sum(0), d.rB[u] - rBp.sum(0)) if ne else np.zeros(0)
            r.xs[u] = np.einsum("kab,kb->ka", r.Dinv, d.rhs[u]) - (r.Z @ xB if ne else 0.0)
            r.xB[u] = xB
        else:
            for sl in lanes:
                r.xs[u, sl], xB = ref.solve(r.Dinv[sl], r.X[sl], r.Y[sl], r.Z[sl], d.G, r.Gp[sl], d.rhs[u, sl], d.rB[u])
            r.xB[u] = xB
    got = np.concatenate([r.xs.reshape(NRHS_MAX, S * nb), r.xB], axis=1)
    r.err_cols = [rel(got[u], r.x_ref[u]) for u in range(NRHS_MAX)]
    r.err_cpu = r.err_cols[0]
    r.bounds = [16.0 * max(e, c.n * 2.0 ** -52) for e in r.err_cols]      # per column: 16 max(err_cpu, n 2^-52), from the reference alone
    r.bound = r.bounds[0]
    r.K = K
    return r
