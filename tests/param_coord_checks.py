"""What the tests of the explicit θ blocks (∂c/∂θ, ∂²L/∂x∂θ, ∂²L/∂θ² in COO) share, on the CPU emulation and on the GPU:
coverage of the output buffers, ranges of the structure, and the identities against the matrix-free kinds.

The identity tolerance is derived, not measured: a product of a COO block with a vector and the matching matrix-free
kind are float64 sums of the SAME products v·w in different orders, so per output entry
``|diff| <= 4·n·ε·Σ|v·w|`` with n the number of addends of the entry, ε = 2⁻⁵² and the sum over those addends."""
import numpy as np

EPS = 2.0 ** -52


def check_coverage(buf, nnz, what):
    """`buf` was NaN before the call: exactly its first `nnz` entries were written, the guard behind them was not"""
    buf = np.asarray(buf)
    assert not np.isnan(buf[:nnz]).any(), f"{what}: {int(np.isnan(buf[:nnz]).sum())} of {nnz} entries never written"
    assert np.isnan(buf[nnz:]).all(), f"{what}: wrote behind the block"
    assert int((~np.isnan(buf)).sum()) == nnz


def check_structure(struct0, struct1, nvar, ncon, npar):
    """`struct0` / `struct1`: the three (rows, cols) pairs with base 0 / base 1"""
    lim = [(ncon, npar), (nvar, npar), (npar, npar)]
    for (r0, c0), (r1, c1), (nr, nc) in zip(struct0, struct1, lim):
        np.testing.assert_array_equal(r1, r0 + 1)
        np.testing.assert_array_equal(c1, c0 + 1)
        if len(r0):
            assert r0.min() >= 0 and r0.max() < nr and c0.min() >= 0 and c0.max() < nc
    r, c = struct0[2]
    assert (r >= c).all()      # the triangle hess_structure uses


def apply(rows, cols, vals, vec, n_out, transpose=False):
    """(A·vec or Aᵀ·vec, Σ|a·vec| per entry, addends per entry) for the COO triplets, in float64 on the host"""
    if transpose:
        rows, cols = cols, rows
    prod = vals * vec[cols]
    out, mag, cnt = np.zeros(n_out), np.zeros(n_out), np.zeros(n_out)
    np.add.at(out, rows, prod)
    np.add.at(mag, rows, np.abs(prod))
    np.add.at(cnt, rows, 1.0)
    return out, mag, cnt


def apply_sym(rows, cols, vals, vec, n):
    """sym(H)·vec where sym mirrors the strict triangle"""
    a, am, ac = apply(rows, cols, vals, vec, n)
    off = rows != cols
    b, bm, bc = apply(rows[off], cols[off], vals[off], vec, n, transpose=True)
    return a + b, am + bm, ac + bc


def assert_identity(got, mag, cnt, want, what):
    want = np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bound = 4.0 * cnt * EPS * mag
    bad = np.abs(got - want) > bound
    assert not bad.any(), (what, int(bad.sum()), float(np.abs(got - want).max()), float(bound[bad].max()) if bad.any() else 0.0)


def check_identities(struct, vals, products, nvar, ncon, npar, rng):
    """`vals`: the three value arrays; `products`: callables jpprod(w), jptprod0(y), hpprod(w), hptprod(u), hppprod(w) of the
    matrix-free kinds at the same (x, y, obj_weight) — jptprod0 with obj_weight = 0 and the y it is given"""
    (jr, jc), (xr, xc), (pr, pc) = struct
    jv, xv, pv = vals
    for _ in range(3):
        w, u, yy = rng.standard_normal(npar), rng.standard_normal(nvar), rng.standard_normal(ncon)
        assert_identity(*apply(jr, jc, jv, w, ncon), products["jpprod"](w), "Jθ·w")
        assert_identity(*apply(jr, jc, jv, yy, npar, True), products["jptprod0"](yy), "Jθᵀ·y")
        assert_identity(*apply(xr, xc, xv, w, nvar), products["hpprod"](w), "Hxθ·w")
        assert_identity(*apply(xr, xc, xv, u, npar, True), products["hptprod"](u), "Hxθᵀ·u")
        assert_identity(*apply_sym(pr, pc, pv, w, npar), products["hppprod"](w), "sym(Hθθ)·w")


def dense(rows, cols, vals, shape, sym=False):
    a = np.zeros(shape)
    np.add.at(a, (rows, cols), vals)
    if sym:
        off = rows != cols
        np.add.at(a, (cols[off], rows[off]), vals[off])
    return a


def probe_classes(patterns, npar):
    """Colour the θ columns so that no row of any pattern in `patterns` (pairs (rows, cols), every one over the θ columns)
    holds two columns of one class: the product of a block with a class's indicator vector then shows every entry of those
    columns by itself.  Greedy, in column order; returns the list of classes (arrays of column indices)."""
    rows_of = [[] for _ in range(npar)]
    for p, (r, c) in enumerate(patterns):
        for ri, ci in zip(r.tolist(), c.tolist()):
            rows_of[ci].append((p, ri))
    taken = []      # per class: the set of (pattern, row) its columns occupy
    classes = []
    for c in range(npar):
        mine = set(rows_of[c])
        for k, occ in enumerate(taken):
            if not (mine & occ):
                occ |= mine
                classes[k].append(c)
                break
        else:
            taken.append(mine)
            classes.append([c])
    return [np.asarray(k, dtype=np.int64) for k in classes]


def check_entries(struct, vals, witness, nvar, ncon, npar, tol, max_classes=24):
    """ENTRY BY ENTRY against the witness's dense blocks: the columns of θ are split into classes no row sees twice
    (probe_classes, on the patterns the structure calls report), so witness·indicator(class) holds, per row, exactly one
    entry of the dense block — or zero where the block has none there, which catches a missing entry.  Hθθ is symmetric:
    its classes come from ONE triangle (the orientation that needs fewer), a row that still sees a class twice through the
    mirrored entries is left out for that class, and every entry must have been seen by itself at (r, c) or at (c, r).
    `witness`: callables jpprod(w), hpprod(w), hppprod(w).  Returns the worst relative gap (relative to max(1, |product|∞))."""
    (jr, jc), (xr, xc), (pr, pc) = struct
    lo, hi = np.maximum(pr, pc), np.minimum(pr, pc)
    classes = min((probe_classes([(jr, jc), (xr, xc), tri], npar) for tri in ((lo, hi), (hi, lo))), key=len)
    assert len(classes) <= max_classes, f"{len(classes)} probe classes: too many products for a quick test"
    blocks = [dense(jr, jc, vals[0], (ncon, npar)), dense(xr, xc, vals[1], (nvar, npar)), dense(pr, pc, vals[2], (npar, npar), sym=True)]
    pattern = np.zeros((npar, npar), dtype=bool)
    pattern[pr, pc] = True
    pattern |= pattern.T
    seen = np.zeros((npar, npar), dtype=bool)
    worst = 0.0
    for cls in classes:
        w = np.zeros(npar)
        w[cls] = 1.0
        for b, (blk, name) in enumerate(zip(blocks, ("jpprod", "hpprod", "hppprod"))):
            want = np.asarray(witness[name](w))
            got = blk[:, cls].sum(axis=1)
            if b < 2:
                rows = np.arange(blk.shape[0])
                assert np.count_nonzero(blk[:, cls], axis=1).max(initial=0) <= 1      # one entry per row and class: entrywise
            else:
                rows = np.flatnonzero(pattern[:, cls].sum(axis=1) <= 1)
                seen[np.ix_(rows, cls)] = True
            if len(rows):
                worst = max(worst, float(np.abs(got[rows] - want[rows]).max() / max(1.0, np.abs(want).max(initial=0.0))))
    assert not (pattern & ~(seen | seen.T)).any(), "an entry of Hθθ was never seen by itself"
    assert worst <= tol, worst
    return worst
