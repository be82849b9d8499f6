"""The sparse sibling of ``test_sympy_reference.SympyModel.dense`` for the operator-domain sweep, and what the CPU test, the
GPU test and tools/op_domain_report.py share to compare an evaluator with it.

Each template is differentiated symbolically once (the ``UN`` table and ``exact()`` of test_sympy_reference.py) and evaluated
per item with 50-digit mpmath arithmetic on the binary64 inputs taken exactly.  The Jacobian and the Lagrangian Hessian (lower
triangle) come back keyed ``(row, col)``: the code under test has its COO output summed per key (``summed``)."""
import math

import mpmath
import numpy as np
import sympy as sp

import cases_op_domain as D
from infiniteexamodels.jl_amd import nodes as N
from infiniteexamodels.jl_amd.core import T_OBJ
from test_sympy_reference import SympyModel

DPS = 50
HARD = 1e-10              # the project's bar (BASELINE.json north_star), purely relative
ULP32 = 32 * 2.0 ** -53   # the floor of the sharp bound
MARGIN = 8.0              # ... and its margin over the oracle's own error at the same element


class Reference:
    """obj / cons / grad as numbers and arrays, jac / hess as sorted key arrays with values; `scale` of an output: what its
    error is relative to (|ref| per element; Σ|term| for obj)."""

    def products(self, v, vc):
        """(value, Σ|addend|) of J·v, Jᵀ·vc and H·v from the reference matrices (exactly rounded sums of the binary64 products)"""
        def acc(n, rows, cols, vals, vec, sym):
            add = [[] for _ in range(n)]
            for r, c, a in zip(rows, cols, vals):
                add[r].append(a * vec[c])
                if sym and r != c:
                    add[c].append(a * vec[r])
            return np.array([math.fsum(t) for t in add]), np.array([math.fsum(abs(u) for u in t) for t in add])
        jr, jc = self.jkeys[:, 0], self.jkeys[:, 1]
        hr, hc = self.hkeys[:, 0], self.hkeys[:, 1]
        return {"jprod": acc(self.ncon, jr, jc, self.jac, v, False), "jtprod": acc(self.nvar, jc, jr, self.jac, vc, False),
                "hprod": acc(self.nvar, hr, hc, self.hess, v, True)}


class SparseSympyModel(SympyModel):
    def __init__(self, core):
        super().__init__(core)
        self._fns = {}

    def expr(self, node, leaves):
        # a constant enters as the exact rational its binary64 value is (exact() at full length): a Float exponent would leave
        # a^2.0 -> 2.0·a^2.0/a in the derivative, which has no value at a = 0
        if isinstance(node, (N.Null, N.Const)):
            return sp.Rational(float(node.value))
        return super().expr(node, leaves)

    def _template(self, ti):
        if ti not in self._fns:
            t = self.core.templates[ti]
            leaves = {}
            e = self.expr(t.expr, leaves)
            keys = list(leaves)
            syms = [leaves[k] for k in keys]
            vs = [i for i, k in enumerate(keys) if k[0] == "v"]
            d1 = [sp.diff(e, syms[i]) for i in vs]
            d2 = [[sp.diff(d, syms[j]) for j in vs] for d in d1]
            mods = [{"DiracDelta": lambda *a: mpmath.mpf(0)}, "mpmath"]
            self._fns[ti] = (keys, vs, sp.lambdify(syms, [e] + d1 + [q for r in d2 for q in r], mods, cse=True))
        return self._fns[ti]

    def evaluate(self, x, y, w, templates=None):
        """`templates`: restrict to these template indices (rows of the others stay NaN in `cons`)."""
        core = self.core
        ref = Reference()
        ref.nvar, ref.ncon = core.nvar, core.ncon
        mp0 = mpmath.mpf(0)
        with mpmath.workdps(DPS):
            cons = np.full(core.ncon, np.nan)
            grad, jac, hess = {}, {}, {}
            f, fabs = mp0, mp0
            for ti, t in enumerate(core.templates):
                if templates is not None and ti not in templates:
                    continue
                keys, vs, fn = self._template(ti)
                nv = len(vs)
                for k in range(len(t.items)):
                    pt = []
                    for kind, key in keys:
                        if kind == "d":
                            pt.append(mpmath.mpf(float(t.items.column(key)[k])))
                        elif kind == "p":
                            pt.append(mpmath.mpf(float(core.theta[self.index(t.items, k, key)])))
                        else:
                            pt.append(mpmath.mpf(float(x[self.index(t.items, k, key)])))
                    out = [mpmath.mpf(v) for v in fn(*pt)]
                    ids = [self.index(t.items, k, keys[i][1]) for i in vs]
                    if t.kind == T_OBJ:
                        f += out[0]
                        fabs += abs(out[0])
                        scale = mpmath.mpf(float(w))
                        for i, v in zip(ids, out[1:1 + nv]):
                            grad[i] = grad.get(i, mp0) + v
                    else:
                        row = t.o0 + k
                        cons[row] = float(out[0])
                        scale = mpmath.mpf(float(y[row]))
                        for i, v in zip(ids, out[1:1 + nv]):
                            jac[(row, i)] = jac.get((row, i), mp0) + v
                    for a in range(nv):
                        for b in range(nv):
                            if ids[a] >= ids[b]:
                                key = (ids[a], ids[b])
                                hess[key] = hess.get(key, mp0) + scale * out[1 + nv + a * nv + b]
            ref.obj, ref.obj_scale = float(f), float(fabs)
            ref.cons = cons
            ref.grad = np.zeros(core.nvar)
            for i, v in grad.items():
                ref.grad[i] = float(v)
            ref.jkeys = np.array(sorted(jac), dtype=np.int64).reshape(-1, 2)
            ref.jac = np.array([float(jac[tuple(k)]) for k in ref.jkeys])
            ref.hkeys = np.array(sorted(hess), dtype=np.int64).reshape(-1, 2)
            ref.hess = np.array([float(hess[tuple(k)]) for k in ref.hkeys])
        return ref


def summed(keys, rows, cols, vals, lower=False):
    """COO output summed per (row, col) [lower triangle: (max, min)], laid out along the reference's sorted `keys`; a key the
    reference has and the structure has not reads 0 (and then has to BE 0), a key the reference lacks is an error."""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    if lower:
        rows, cols = np.maximum(rows, cols), np.minimum(rows, cols)
    big = int(max(keys[:, 1].max(), cols.max())) + 1
    flat = keys[:, 0] * big + keys[:, 1]
    pos = np.searchsorted(flat, rows * big + cols)
    assert (pos < flat.size).all() and (flat[pos] == rows * big + cols).all(), "a structural entry the reference does not have"
    out = np.zeros(flat.size)
    np.add.at(out, pos, np.asarray(vals, dtype=np.float64))
    return out


class Evaluator:
    """The entry points of one evaluator as numpy arrays (subclasses: the oracle, the emulated kernels, the GPU)."""

    def __init__(self, om):
        self.om = om
        self.jr, self.jc = om.jac_structure()
        self.hr, self.hc = om.hess_structure()


class OracleEval(Evaluator):
    name = "oracle"

    def obj(self, x): return self.om.obj(x)
    def cons(self, x): return self.om.cons(x)
    def grad(self, x): return self.om.grad(x)
    def jac_coord(self, x): return self.om.jac_coord(x)
    def hess_coord(self, x, y, w): return self.om.hess_coord(x, y, w)
    def jprod(self, x, v): return self.om.jprod(x, v)
    def jtprod(self, x, v): return self.om.jtprod(x, v)
    def hprod(self, x, y, v, w): return self.om.hprod(x, y, v, w)
    def set_theta(self, value): self.om.set_parameter(0, [value])


class EmuEval(Evaluator):
    name = "emulator"

    def __init__(self, om, em):
        super().__init__(om)
        self.em = em

    def obj(self, x): return self.em.obj(x)
    def cons(self, x): return self.em.cons(x)
    def grad(self, x): return self.em.grad(x)
    def jac_coord(self, x): return self.em.jac_coord(x, self.om.nnzj)
    def hess_coord(self, x, y, w): return self.em.hess_coord(x, y, w, self.om.nnzh)
    def jprod(self, x, v): return self.em.jprod(x, v)
    def jtprod(self, x, v): return self.em.jtprod(x, v)
    def hprod(self, x, y, v, w): return self.em.hprod(x, y, v, w)
    def set_theta(self, value): self.em.theta[0] = value


SIGMA = 0.7


def sweep_inputs(model, core, seed=1):
    """x, y (random, non-zero, of one sign: the rows of a slab must not cancel in its Hessian entry), v, vc"""
    rng = np.random.default_rng(seed + 100)
    x = D.points(model, seed)
    y = rng.uniform(0.5, 1.5, core.ncon)
    return x, y, rng.standard_normal(core.nvar), rng.standard_normal(core.ncon)


def outputs(ev, ref, x, y, v, vc):
    """name -> (got, reference, scale) along the reference's layout, for everything the sweep checks"""
    prods = ref.products(v, vc)
    out = {
        "obj": (np.array([ev.obj(x)]), np.array([ref.obj]), np.array([ref.obj_scale])),
        "cons": (ev.cons(x), ref.cons, np.abs(ref.cons)),
        "grad": (ev.grad(x), ref.grad, np.abs(ref.grad)),
        "jac_coord": (summed(ref.jkeys, ev.jr, ev.jc, ev.jac_coord(x)), ref.jac, np.abs(ref.jac)),
        "hess_coord": (summed(ref.hkeys, ev.hr, ev.hc, ev.hess_coord(x, y, SIGMA), lower=True), ref.hess, np.abs(ref.hess)),
        "jprod": (ev.jprod(x, v),) + prods["jprod"],
        "jtprod": (ev.jtprod(x, vc),) + prods["jtprod"],
        "hprod": (ev.hprod(x, y, v, SIGMA),) + prods["hprod"],
    }
    return out


def owners(model, ref, what):
    """(operator or form, item) of every element of output `what`; a Hessian entry between a slab and the shared `b` belongs to
    the slab"""
    if what in ("cons", "jprod"):
        return [D.owner_of_row(model, r) for r in range(ref.ncon)]
    if what in ("grad", "jtprod", "hprod"):
        return [D.owner_of_col(model, c) for c in range(ref.nvar)]
    if what == "jac_coord":
        return [D.owner_of_row(model, r) for r in ref.jkeys[:, 0]]
    if what == "hess_coord":
        return [D.owner_of_col(model, c) for c in ref.hkeys[:, 1]]
    return [("obj", 0)]


def label(model, regions, owner):
    op, i = owner
    return f"{op}[{regions[op][i]}] item {i}" if op in regions else f"{op} item {i}"


def check(model, ref, out, regions, e_oracle=None, exceptions=()):
    """The two assertions of the sweep, per output element.  Hard: |got - ref| <= 1e-10·scale, no floor, no exception.  Sharp
    (`e_oracle`: what -> the fixed oracle's own |error| against the same reference at the same element):
    |got - ref| <= max(8·e_oracle, 32·2⁻⁵³·scale), except for the operators of `exceptions`.  Returns the failures as text."""
    bad = []
    for what, (got, r, scale) in out.items():
        got = np.asarray(got, dtype=np.float64)
        assert got.shape == r.shape, what
        err = np.abs(got - r)
        err = np.where(np.isnan(err), np.inf, err)
        own = None
        for k in np.flatnonzero(~(err <= HARD * scale)):
            own = own or owners(model, ref, what)
            bad.append(f"HARD {what} {label(model, regions, own[k])}: got {got[k]!r} ref {r[k]!r} rel {err[k] / scale[k] if scale[k] else np.inf:.3e}")
        if e_oracle is not None:
            lim = np.maximum(MARGIN * e_oracle[what], ULP32 * scale)
            for k in np.flatnonzero(~(err <= lim)):
                own = own or owners(model, ref, what)
                if own[k][0] in exceptions:
                    continue
                bad.append(f"SHARP {what} {label(model, regions, own[k])}: got {got[k]!r} ref {r[k]!r} err {err[k] / scale[k] * 2.0 ** 53:.1f}·2⁻⁵³, "
                           f"oracle {e_oracle[what][k] / scale[k] * 2.0 ** 53:.1f}·2⁻⁵³")
    return bad


def errors_of(out):
    return {what: np.abs(np.asarray(got, dtype=np.float64) - r) for what, (got, r, scale) in out.items()}


def worst_by_owner(model, ref, out):
    """{operator or form: {output: worst relative error}} — the table of DESIGN.md / profiles/op_domain_errors.json"""
    table = {}
    for what, (got, r, scale) in out.items():
        err = np.abs(np.asarray(got, dtype=np.float64) - r)
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.where(err == 0, 0.0, err / scale)
        rel = np.where(np.isnan(rel), np.inf, rel)
        for (op, _), e in zip(owners(model, ref, what), rel):
            d = table.setdefault(op, {})
            d[what] = max(d.get(what, 0.0), float(e))
    return table


# ---- raw COO attribution -------------------------------------------------------------------------------------------------------
def item_masks(om, templates, item):
    """Boolean masks over cons / jac_coord / hess_coord (raw COO): the elements that templates `templates` write for `item`."""
    mc, mj, mh = np.zeros(om.ncon, bool), np.zeros(om.nnzj, bool), np.zeros(om.nnzh, bool)
    for t in templates:
        info = om.template_info(t)
        if info["kind"] != T_OBJ:
            mc[info["o0"] + item] = True
            mj[info["o1"] + info["o1step"] * item: info["o1"] + info["o1step"] * (item + 1)] = True
        mh[info["o2"] + info["o2step"] * item: info["o2"] + info["o2step"] * (item + 1)] = True
    return mc, mj, mh


def klass(a):
    """0 finite, 1 NaN, 2 +inf, 3 -inf"""
    a = np.asarray(a, dtype=np.float64)
    return np.where(np.isnan(a), 1, np.where(np.isposinf(a), 2, np.where(np.isneginf(a), 3, 0)))


# ---- the sweep's cases, computed once per process ------------------------------------------------------------------------------
_CASES = {}


def sweep_case(model):
    """core, blob, the oracle's evaluator, the inputs, the reference, the oracle's outputs and its errors — shared by every
    test of the process and left unchanged"""
    if model not in _CASES:
        from types import SimpleNamespace
        from pyoracle import OracleModel
        core = D.build_core(model)
        blob = core.to_blob()
        oe = OracleEval(OracleModel(blob))
        x, y, v, vc = sweep_inputs(model, core)
        sym = SparseSympyModel(core)
        ref = sym.evaluate(x, y, SIGMA)
        out = outputs(oe, ref, x, y, v, vc)
        _CASES[model] = SimpleNamespace(model=model, core=core, blob=blob, oe=oe, x=x, y=y, v=v, vc=vc, sym=sym, ref=ref, out_oracle=out,
                                        e_oracle=errors_of(out), regions=D.region_names(model))
    return _CASES[model]


def sweep_failures(case, ev, sharp=True, exceptions=()):
    out = outputs(ev, case.ref, case.x, case.y, case.v, case.vc)
    return check(case.model, case.ref, out, case.regions, case.e_oracle if sharp else None, exceptions)


# ---- a^θ₀ with the exponent set at run time ------------------------------------------------------------------------------------
def theta_failures(case, ev, sharp=True):
    """`case` of binary_sweep: θ₀ through D.THETAS, the rows / Jacobian / Hessian entries of the form a^θ₀ against the reference"""
    k = D.FORMS.index("a^theta")
    rows = np.arange(case.core.ncon) // D.N == k

    def outs(e, ref):
        jm, hm = e.jr // D.N == k, e.hc // D.N // 2 == k
        return {"cons": (np.where(rows, e.cons(case.x), 0.0), ref.cons, np.abs(ref.cons)),
                "jac_coord": (summed(ref.jkeys, e.jr[jm], e.jc[jm], e.jac_coord(case.x)[jm]), ref.jac, np.abs(ref.jac)),
                "hess_coord": (summed(ref.hkeys, e.hr[hm], e.hc[hm], e.hess_coord(case.x, case.y, SIGMA)[hm], lower=True), ref.hess, np.abs(ref.hess))}
    bad = []
    try:
        for th in D.THETAS:
            case.core.theta[case.core.theta_par.offset] = th      # (the reference reads the core's θ)
            case.oe.set_theta(th)
            ev.set_theta(th)
            ref = case.sym.evaluate(case.x, case.y, SIGMA, templates=[k])
            ref.cons = np.where(rows, ref.cons, 0.0)
            e_or = errors_of(outs(case.oe, ref))
            bad += [f"theta = {th}: {b}" for b in check(case.model, ref, outs(ev, ref), case.regions, e_or if sharp else None)]
    finally:
        case.core.theta[case.core.theta_par.offset] = D.THETAS[0]
        case.oe.set_theta(D.THETAS[0])
        ev.set_theta(D.THETAS[0])
    return bad


# ---- special points ------------------------------------------------------------------------------------------------------------
def _raw(ev, x, ncon):
    """cons, jac_coord, hess_coord (y = 1, σ = 1: a raw Hessian entry of a one-row template IS f'') as written"""
    return ev.cons(x), ev.jac_coord(x), ev.hess_coord(x, np.ones(ncon), 1.0)


def _agree(name, got, want, bad):
    """class for class the oracle's; where that is finite, its value to the bar"""
    kg, kw = klass(got), klass(want)
    for i in np.flatnonzero(kg != kw):
        bad.append(f"{name}[{i}]: {got[i]!r}, the oracle has {want[i]!r}")
    fin = (kg == 0) & (kw == 0)
    with np.errstate(invalid="ignore"):
        off = fin & ~(np.abs(got - want) <= HARD * np.abs(want))
    for i in np.flatnonzero(off):
        bad.append(f"{name}[{i}]: {got[i]!r}, the oracle has {want[i]!r}")


def _exact(what, fdh, want, bad):
    for part, g, w in zip(("f", "f'", "f''"), fdh, want):
        if w is not None and not g == w:
            bad.append(f"{what}: {part} = {g!r}, the limit is {w!r}")


def special_failures(case, ev):
    """The second, exact point: the finite limits exactly (on `ev`; pass the oracle's evaluator to hold the oracle to them),
    every element's class and finite value as the oracle's."""
    model, om, bad = case.model, case.oe.om, []
    x = D.special_points(model)
    got, want = _raw(ev, x, om.ncon), _raw(case.oe, x, om.ncon)
    for name, g, w in zip(("cons", "jac_coord", "hess_coord"), got, want):
        _agree(name, np.asarray(g), np.asarray(w), bad)

    def fdh(tpl, item):
        info = om.template_info(tpl)
        assert info["o1step"] >= 1 and info["o2step"] >= 1
        return got[0][info["o0"] + item], got[1][info["o1"] + info["o1step"] * item], got[2][info["o2"] + info["o2step"] * item]
    if model == "unary_sweep":
        for op, pts in D.SPECIAL_UNARY.items():
            for j, (v, want_fdh) in enumerate(pts):
                if want_fdh is not None:
                    _exact(f"{op}({v!r})", fdh(D.OPS.index(op), j), want_fdh, bad)
    else:
        for form, want_fdh in D.SPECIAL_BINARY.items():
            if want_fdh is not None:
                _exact(f"{form} at a = 0", fdh(D.FORMS.index(form), 0), want_fdh, bad)
    return bad


def theta_zero_base_failures(case, ev):
    """a^θ₀ at a = 0 has the reference's formula and no folding: θ₀·(θ₀ - 1)·0^(θ₀ - 2) is 0·inf = NaN for θ₀ in {0, 1}, in the
    kernels as in the oracle; pinned, not judged"""
    om, bad = case.oe.om, []
    k = D.FORMS.index("a^theta")
    x = D.special_points(case.model)
    info = om.template_info(k)
    try:
        for th in (0.0, 1.0):
            case.oe.set_theta(th)
            ev.set_theta(th)
            got, want = _raw(ev, x, om.ncon), _raw(case.oe, x, om.ncon)
            for name, g, w in zip(("cons", "jac_coord", "hess_coord"), got, want):
                _agree(f"theta = {th}: {name}", np.asarray(g), np.asarray(w), bad)
            h = np.asarray(got[2])[info["o2"]: info["o2"] + info["o2step"] * D.N]
            if not np.isnan(h).all():
                bad.append(f"theta = {th}: f'' of a^theta at a = 0 is no longer NaN everywhere")
    finally:
        case.oe.set_theta(D.THETAS[0])
        ev.set_theta(D.THETAS[0])
    return bad


# ---- one bad lane ----------------------------------------------------------------------------------------------------------------
BAD_ITEM = 70        # mid-wavefront, not the first of its block
BAD_LANES = (("log", -1.0), ("sqrt", -1.0), ("asin", 2.0))


def bad_lane_failures(case, ev, op, value):
    """One item of the unary model moved out of its operator's domain: every element of cons / jac_coord / hess_coord that
    does not belong to that item carries the BITS of the in-domain run; the item's own are NaN exactly where the oracle's are."""
    om, bad = case.oe.om, []
    x = case.x.copy()
    x[D.OPS.index(op) * D.N + BAD_ITEM] = value
    masks = item_masks(om, D.templates_of(case.model, op), BAD_ITEM)
    good = (ev.cons(case.x), ev.jac_coord(case.x), ev.hess_coord(case.x, case.y, SIGMA))
    got = (ev.cons(x), ev.jac_coord(x), ev.hess_coord(x, case.y, SIGMA))
    want = (case.oe.cons(x), case.oe.jac_coord(x), case.oe.hess_coord(x, case.y, SIGMA))
    for name, m, a, g, w in zip(("cons", "jac_coord", "hess_coord"), masks, good, got, want):
        a, g, w = (np.ascontiguousarray(t, dtype=np.float64) for t in (a, g, w))
        assert m.any()
        moved = np.flatnonzero((a.view(np.int64) != g.view(np.int64)) & ~m)
        if moved.size:
            bad.append(f"{op}({value}) at item {BAD_ITEM}: {moved.size} foreign elements of {name} moved, first {moved[0]}: {a[moved[0]]!r} -> {g[moved[0]]!r}")
        if not np.array_equal(np.isnan(g[m]), np.isnan(w[m])):
            bad.append(f"{op}({value}) at item {BAD_ITEM}: NaN pattern of the item's own {name} {np.isnan(g[m]).tolist()}, the oracle's {np.isnan(w[m]).tolist()}")
        if name == "cons" and not np.isnan(g[m]).all():      # (log'(-1) and log''(-1) are finite: only the value has to be NaN)
            bad.append(f"{op}({value}) at item {BAD_ITEM}: the item's own rows are not NaN")
    return bad
