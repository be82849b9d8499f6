"""numpy restatement of csrc/iem_kkt_diag_device.h — kkt_gather_d, kkt_residual_dm, kkt_axpy_m, expression for expression (numpy
rounds every operation and contracts nothing: what -ffp-contract=off makes of the kernels) — and the inputs the tests of the
per-row diagonal share.  TEST INFRASTRUCTURE: tests/test_kkt_diag.py (CPU) and tests/test_gpu_kkt_diag.py."""
import numpy as np

DW, DC = 1e-2, 1e-6


def gather_sources(hess, jac, sigma, dcon, dw, dc, nvar, ncon):
    """the virtual array the gather plan indexes:  hess | jac | sigma + dw per variable | −(dcon + dc) per row | 1.0"""
    per_var = (np.zeros(nvar) if sigma is None else np.asarray(sigma, dtype=np.float64)) + dw
    per_row = -(np.asarray(dcon, dtype=np.float64) + dc) if dcon is not None else np.full(ncon, -dc)
    return np.concatenate([hess, jac, per_var, per_row, [1.0]])


def gather(total, dest, seg, perm, src):
    """flat[dest[i]] = the sum, in the order of the plan, of src[perm[seg[i] : seg[i + 1]]] (starting from +0.0, as the kernel does)"""
    flat = np.zeros(total)
    vals = np.zeros(len(dest))
    seg = np.asarray(seg, dtype=np.int64)
    width = int(np.diff(seg).max()) if len(dest) else 0
    for j in range(width):              # term j of every segment that has one: the kernel's loop, vectorised over the destinations
        has = seg[:-1] + j < seg[1:]
        vals[has] = vals[has] + src[perm[seg[:-1][has] + j]]
    flat[dest] = vals
    return flat


def residual_dm(p, rhs, sol, sigma, dcon, dw, dc, nvar):
    """``(r, norms)`` for columns held as rows of (K, n) arrays: r_x = rhs − (p + ((sigma | 0) + dw)·sol),
    d = dcon + dc (dc alone without dcon), r_y = rhs − (p − d·sol); norms[u] = max |r_u| with a NaN giving a NaN."""
    p, rhs, sol = (np.atleast_2d(np.asarray(a, dtype=np.float64)) for a in (p, rhs, sol))
    n = p.shape[1]
    dx = (np.zeros(nvar) if sigma is None else np.asarray(sigma, dtype=np.float64)) + dw
    dy = np.asarray(dcon, dtype=np.float64) + dc if dcon is not None else np.full(n - nvar, dc)
    t = np.empty_like(p)
    t[:, :nvar] = p[:, :nvar] + dx * sol[:, :nvar]
    t[:, nvar:] = p[:, nvar:] - dy * sol[:, nvar:]
    r = rhs - t
    with np.errstate(invalid="ignore"):
        norms = np.abs(r).max(axis=1) if n else np.zeros(r.shape[0])      # (numpy's max propagates a NaN, as the maximum on the bit patterns does)
    return r, norms


def axpy_m(sol, d):
    return np.asarray(sol, dtype=np.float64) + np.asarray(d, dtype=np.float64)


def diag_inputs(nvar, ncon):
    """``(sigma, dcon, rhs)`` of the tests: sigma = 0.5 + U(0, 1); dcon = 0 except on the rows drawn with probability 1/2, which get
    10^U(−8, 8) — sixteen decades of Sigma_s^-1, rows without an inequality in between; default_rng(3)."""
    rng = np.random.default_rng(3)
    sigma = 0.5 + rng.random(nvar)
    on = rng.random(ncon) < 0.5
    dcon = np.where(on, 10.0 ** rng.uniform(-8.0, 8.0, ncon), 0.0)
    return sigma, dcon, rng.standard_normal(nvar + ncon)


def host_kkt_diag(om, x, y, sigma, dw, dcon_plus_dc, w=1.0):
    """scipy's  [[H + diag(sigma + dw), J'], [J, −diag(dcon + dc)]]  from the oracle's values"""
    import scipy.sparse as sp
    n, m = om.nvar, om.ncon
    hr, hc = om.hess_structure()
    jr, jc = om.jac_structure()
    L = sp.coo_matrix((om.hess_coord(x, y, w), (hr, hc)), shape=(n, n)).tocsr()
    H = L + L.T - sp.diags(L.diagonal())
    J = sp.coo_matrix((om.jac_coord(x), (jr, jc)), shape=(m, n)).tocsr()
    return sp.bmat([[H + sp.diags(sigma + dw), J.T], [J, -sp.diags(np.broadcast_to(dcon_plus_dc, (m,)))]]).tocsr()


_systems = {}


def host_system(name, w=1.0):
    """``dict(core, blob, om, x, y, sigma, dcon, rhs, K, neg)`` at ``cases.eval_point_for(name, om, 5)``: built once per model and
    process, shared by the tests and left unchanged.  ``neg``: the negative eigenvalues of K (None beyond 4000 unknowns)."""
    if (name, w) not in _systems:
        import cases
        from pyoracle import OracleModel
        core = cases.build_core(name)
        blob = core.to_blob()
        om = OracleModel(blob)
        x, y = cases.eval_point_for(name, om, 5)
        sigma, dcon, rhs = diag_inputs(om.nvar, om.ncon)
        K = host_kkt_diag(om, x, y, sigma, DW, dcon + DC, w)
        K.sum_duplicates(); K.sort_indices()
        n = om.nvar + om.ncon
        neg = int((np.linalg.eigvalsh(K.toarray()) < 0).sum()) if n <= 4000 else None
        _systems[name, w] = dict(core=core, blob=blob, om=om, x=x, y=y, sigma=sigma, dcon=dcon, rhs=rhs, K=K, neg=neg)
    return _systems[name, w]


def residual_ok(K, sol, rhs):
    """the project's criterion for a refined solve: ‖K·sol − rhs‖∞ <= 1e-9·max(1, ‖rhs‖∞), or componentwise <= 1e-12"""
    resid = np.abs(K @ sol - rhs)
    with np.errstate(invalid="ignore", divide="ignore"):
        comp = (resid / (abs(K) @ np.abs(sol) + np.abs(rhs))).max()
    return bool(resid.max() <= 1e-9 * max(1.0, np.abs(rhs).max()) or comp <= 1e-12), float(resid.max()), float(comp)
