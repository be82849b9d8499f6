"""numpy restatement of the dense border's kernels (csrc/iem_kkt_border_device.h), operation for operation and in the kernels'
order: the two-launch column sum, ``kkt_border_ldl`` (Bunch–Kaufman LDLᵀ with partial pivoting, the same pivot rule, tie break,
update expressions, counting and doubtful handling) and ``kkt_border_solve``.  Everything is IEEE double arithmetic without
contraction, so a GPU result can be compared bit for bit.  Also here: the matrix families of the tests and the restated rule of
``iem::sym_inertia_ldl`` (the host path's inertia for borders beyond 64)."""
import numpy as np

ALPHA = 0.6403882032022076      # (1 + sqrt(17)) / 8, the literal of the kernel
REL = 1e-14


def colsum(a):
    """Column sums of a (rows, w) array as ``kkt_colsum_m`` / ``kkt_border_colsum`` form them: up to 512 chunks of rows, each summed from 0.0 in row
    order, then the partial rows summed from 0.0 in chunk order."""
    a = np.asarray(a, dtype=np.float64)
    rows, w = a.shape
    per = (rows + 511) // 512
    nrc = (rows + per - 1) // per
    part = np.zeros((nrc, w))
    for c in range(nrc):
        acc = np.zeros(w)
        for r in range(c * per, min((c + 1) * per, rows)):
            acc = acc + a[r]
        part[c] = acc
    out = np.zeros(w)
    for c in range(nrc):
        out = out + part[c]
    return out


def _argmax_first(v):
    """(max, lowest index of it) of a non-empty vector of absolute values"""
    i = int(np.argmax(v))
    return float(v[i]), i


def ldl(G, gsum=None, rel=REL):
    """``kkt_border_ldl``: returns ``(F, piv, negative, doubtful, n2x2)``."""
    n = G.shape[0]
    A = np.array(G, dtype=np.float64) - (np.zeros((n, n)) if gsum is None else np.asarray(gsum, dtype=np.float64).reshape(n, n))
    scale = float(np.max(np.abs(A))) if n else 0.0
    thr = rel * scale
    perm = list(range(n))
    typ = [0] * n
    neg = dbt = n2 = 0
    k = 0
    with np.errstate(all="ignore"):
        while k < n:
            akk = A[k, k]
            absakk = abs(akk)
            if k + 1 < n:
                colmax, imax = _argmax_first(np.abs(A[k + 1:, k]))
                imax += k + 1
            else:
                colmax, imax = 0.0, -1
            if scale == 0.0 or (absakk <= thr and colmax <= thr):
                A[k, k] = np.copysign(thr, akk)
                A[k + 1:, k] = 0.0
                dbt += 1
                k += 1
                continue
            kp, kstep = k, 1
            if not (absakk >= ALPHA * colmax):
                dimax = abs(A[imax, imax])
                rowmax = max(float(np.max(np.abs(A[imax, k:imax]))) if imax > k else -1.0,
                             float(np.max(np.abs(A[imax + 1:, imax]))) if imax + 1 < n else -1.0)
                if absakk >= ALPHA * colmax * (colmax / rowmax):
                    kp = k
                elif dimax >= ALPHA * rowmax:
                    kp = imax
                else:
                    kp, kstep = imax, 2
            kk = k + kstep - 1
            if kp != kk:      # rows / columns kk < kp of the lower triangle change places, the finished columns of L with them
                for j in range(n):
                    if j < kk:
                        a, b = (kk, j), (kp, j)
                    elif j == kk:
                        a, b = (kk, kk), (kp, kp)
                    elif j < kp:
                        a, b = (j, kk), (kp, j)
                    elif j == kp:
                        continue
                    else:
                        a, b = (j, kk), (j, kp)
                    A[a], A[b] = A[b], A[a]
                perm[kk], perm[kp] = perm[kp], perm[kk]
            j0 = k + kstep
            if kstep == 1:
                d = A[k, k]
                if d < 0.0:
                    neg += 1
                w1 = A[j0:, k] / d
                # a_ij <- a_ij - a_ik w_j on the lower triangle
                upd = A[j0:, j0:] - np.outer(A[j0:, k], w1)
            else:
                e, dkk, dk1 = A[k + 1, k], A[k, k], A[k + 1, k + 1]
                d11 = dk1 / e
                d22 = dkk / e
                tt = 1.0 / (d11 * d22 - 1.0)
                es = tt / e
                ajk, ajk1 = A[j0:, k].copy(), A[j0:, k + 1].copy()
                w1 = es * (d11 * ajk - ajk1)
                w2 = es * (d22 * ajk1 - ajk)
                det = dkk * dk1 - e * e
                if det < 0.0:
                    neg += 1
                elif dkk < 0.0:
                    neg += 2
                typ[k], typ[k + 1] = 1, 2
                n2 += 1
                upd = (A[j0:, j0:] - np.outer(ajk, w1)) - np.outer(ajk1, w2)
            low = np.tril_indices(n - j0)
            A[j0:, j0:][low] = upd[low]
            A[j0:, k] = w1
            if kstep == 2:
                A[j0:, k + 1] = w2
            k += kstep
    F = np.tril(A)
    piv = np.array([perm[i] if typ[i] == 0 else -(perm[i] + 1) if typ[i] == 1 else -(perm[i] + 1) - n for i in range(n)], dtype=np.int32)
    return F, piv, neg, dbt, n2


def decode(piv):
    """``(perm, typ)`` of a pivot vector: typ 0 a 1×1 pivot, 1 / 2 the first / second row of a 2×2 pivot"""
    n = len(piv)
    perm, typ = [], []
    for p in piv:
        p = int(p)
        t = 0
        if p < 0:
            p, t = -p - 1, 1
            if p >= n:
                p, t = p - n, 2
        perm.append(p)
        typ.append(t)
    return perm, typ


def solve(F, piv, r):
    """``kkt_border_solve`` for one column: x = Pᵀ L⁻ᵀ D⁻¹ L⁻¹ P r (``r`` already rB − column sum)."""
    n = F.shape[0]
    perm, typ = decode(piv)
    with np.errstate(all="ignore"):
        x = np.array([r[perm[i]] for i in range(n)], dtype=np.float64)
        for k in range(n - 1):
            xk = x[k]
            for i in range(k + 1, n):
                if typ[i] == 2 and k == i - 1:
                    continue
                x[i] = x[i] - F[i, k] * xk
        z = x.copy()
        for i in range(n):
            if typ[i] == 0:
                x[i] = z[i] / F[i, i]
            else:
                i0 = i if typ[i] == 1 else i - 1
                e = F[i0 + 1, i0]
                akm1 = F[i0, i0] / e
                ak = F[i0 + 1, i0 + 1] / e
                denom = akm1 * ak - 1.0
                bkm1 = z[i0] / e
                bk = z[i0 + 1] / e
                x[i] = (ak * bkm1 - bk) / denom if typ[i] == 1 else (akm1 * bk - bkm1) / denom
        for k in range(n - 1, 0, -1):
            xk = x[k]
            for i in range(k):
                if typ[i] == 1 and k == i + 1:
                    continue
                x[i] = x[i] - F[k, i] * xk
    out = np.zeros(n)
    for i in range(n):
        out[perm[i]] = x[i]
    return out


def border_rhs(rB, rBp, ne, n_border):
    """r = rB (entries from n_border on taken as zero) − column sum of rBp (S, ne), as the solve kernel forms it"""
    r = np.zeros(ne)
    r[:n_border] = np.asarray(rB)[:n_border]
    return r - colsum(np.asarray(rBp).reshape(-1, ne))


def sym_inertia_ldl(a, rel=REL):
    """``iem::sym_inertia_ldl`` restated (csrc/iem_kkt_host.hpp): LDLᵀ with diagonal pivoting, no 2×2 pivots; ``(neg, doubtful)``"""
    a = np.array(a, dtype=np.float64)
    n = a.shape[0]
    done = [False] * n
    scale = float(np.max(np.abs(np.diag(a)))) if n else 0.0
    neg = dbt = 0
    for _ in range(n):
        p = -1
        for i in range(n):
            if not done[i] and (p < 0 or abs(a[i, i]) > abs(a[p, p])):
                p = i
        d = a[p, p]
        done[p] = True
        if abs(d) <= rel * scale or d == 0.0:
            dbt += 1
            continue
        if d < 0.0:
            neg += 1
        for i in range(n):
            if done[i]:
                continue
            f = a[i, p] / d
            if f == 0.0:
                continue
            for j in range(n):
                if not done[j]:
                    a[i, j] -= f * a[p, j]
    return neg, dbt


# ---- matrix families ------------------------------------------------------------------------------------------------------------
def pad(M, ne):
    """M in the leading block of an ne × ne matrix with the padding's unit diagonal"""
    n = M.shape[0]
    out = np.eye(ne)
    out[:n, :n] = M
    return out


def quasi_definite(n, seed):
    """(a) [A Bᵀ; B −C] with A, C SPD: exactly n − n // 2 positive and n // 2 negative eigenvalues"""
    rng = np.random.default_rng(seed)
    q = n // 2
    p = n - q
    X = rng.standard_normal((p, p))
    Y = rng.standard_normal((q, q))
    B = rng.standard_normal((q, p))
    M = np.zeros((n, n))
    M[:p, :p] = X @ X.T + p * np.eye(p)
    M[p:, p:] = -(Y @ Y.T + q * np.eye(q))
    M[p:, :p] = B
    M[:p, p:] = B.T
    return M, q


def saddle(n, seed, eps=1e-3):
    """(b) [0 B; Bᵀ 0] (n even, B well conditioned) and the same plus a small symmetric perturbation: n / 2 negative eigenvalues"""
    rng = np.random.default_rng(seed)
    h = n // 2
    B = rng.standard_normal((h, h)) + 3.0 * np.eye(h)
    M0 = np.zeros((n, n))
    M0[:h, h:] = B
    M0[h:, :h] = B.T
    P = rng.standard_normal((n, n))
    return M0, M0 + eps * (P + P.T), h


SINGULAR3 = np.array([[2.0, 1.0, 3.0], [1.0, 1.0, 2.0], [3.0, 2.0, 5.0]])      # row 3 = row 1 + row 2: elimination is exact


def singular(n):
    """(c) copies of the exactly singular integer block down the diagonal (n a multiple of 3, or the rest a unit diagonal)"""
    M = np.eye(n)
    for b in range(n // 3):
        M[3 * b:3 * b + 3, 3 * b:3 * b + 3] = SINGULAR3
    return M
