"""Two hand-built models that sweep the operator table (Sweep::unary / Sweep::binary of csrc/iem_codegen.cpp, un_eval /
bin_partials of oracle/iem_oracle.c) over each operator's whole domain, and the evaluation points that do the sweeping.

  * ``unary_sweep``: every operator of ``nodes.UNARY_OPS`` (``neg`` and ``pos`` included) over its own variable slab
    ``v_op``: a constraint row ``f(v_op[i])``, the zoo's composite ``f(v_op[i])·b[i] + f(s·v_op[i])`` over a shared slab
    ``b`` (y1 / h11 travel through products), and an objective template ``f(v_op[i])`` (the gradient's reverse sweep).
    ``s = 0.5`` as in ``cases.operator_zoo`` — except for ``acoth``, whose domain ``|x| > 1`` halving leaves (the zoo keeps
    ``acoth`` out of its composite for that reason): there ``s = 2``.
  * ``binary_sweep``: one constraint row per form of ``BINARY_FORMS`` (constant, real-base and variable exponents, products
    and quotients, the same variable on both sides, a unary of a product, a run-time θ exponent).  Every form reads slabs
    ``a`` and ``b`` OF ITS OWN: the forms have different domains (``a^2.5`` wants ``a >= 0``, ``asin(a·b)`` wants
    ``|a·b| < 1``), and a row that is NaN at an item would poison every sum (Hessian entry, jtprod, hprod) it shares a
    variable with.

Both have ``N = 320`` items: five wavefronts, one full 256-thread workgroup plus a 64-lane tail.

``points(model, seed)`` tiles the named regions of an operator (``unary_regions``) or form (``BINARY_FORMS``) cyclically
over the items, each region with fresh seeded draws.  A region is listed only where every output of the rows that read the
slab is real and finite: the tables here do the dropping, no test does.

These models are NOT part of ``cases.small_cases()``."""
import math

import numpy as np

from infiniteexamodels.jl_amd.core import ExaCore
from infiniteexamodels.jl_amd.items import Items
from infiniteexamodels.jl_amd.nodes import UNARY_OPS, DataSource, Unary

N = 320
OPS = tuple(UNARY_OPS)
THETAS = (2.0, 1.0, 0.0, 3.0, -1.0)      # what the run-time exponent θ₀ is set to, in turn


def half_scale(op):
    return 2.0 if op == "acoth" else 0.5


def _items():
    return Items.from_supports("i", N, {"t": np.linspace(0.0, 1.0, N)}, group_id=1)


def unary_sweep():
    """Variables: slab k (of OPS[k]) at k·N, ``b`` at len(OPS)·N.  Rows: ``f`` of OPS[k] at k·N + i, the composite at
    (len(OPS) + k)·N + i.  Templates: k, len(OPS) + k, 2·len(OPS) + k (objective)."""
    core = ExaCore()
    ds, it = DataSource(), _items()
    slabs = [core.add_var(N, start=2.0 if op == "acoth" else 0.5) for op in OPS]
    b = core.add_var(N, start=1.5)
    for op, v in zip(OPS, slabs):
        core.add_con(Unary(op, v[ds.i]), it)
    for op, v in zip(OPS, slabs):
        core.add_con(Unary(op, v[ds.i]) * b[ds.i] + Unary(op, half_scale(op) * v[ds.i]), it)
    for op, v in zip(OPS, slabs):
        core.add_obj(Unary(op, v[ds.i]), it)
    return core


# name, expression of (a, b, θ₀), regions
BINARY_FORMS = (
    ("a^2", lambda a, b, th: a ** 2, "pp np zero big"),
    ("a^3", lambda a, b, th: a ** 3, "pp np zero big"),
    ("a^-2", lambda a, b, th: a ** -2, "pp np big"),
    ("a^1", lambda a, b, th: a ** 1, "pp np zero big"),
    ("a^0", lambda a, b, th: a ** 0, "pp np zero big"),
    ("a^0.5", lambda a, b, th: a ** 0.5, "pp big"),                      # f' = inf at a = 0
    ("a^2.5", lambda a, b, th: a ** 2.5, "pp zero big"),
    ("2.0^a", lambda a, b, th: 2.0 ** a, "pp np zero"),                 # big: beyond the overflow point
    ("0.5^a", lambda a, b, th: 0.5 ** a, "pp np zero"),
    ("a^b", lambda a, b, th: a ** b, "pp big"),                         # log(a) in the b-partials
    ("(a*b)^3", lambda a, b, th: (a * b) ** 3, "pp np nn zero big"),
    ("a/b", lambda a, b, th: a / b, "pp np nn zero big"),
    ("3.0/b", lambda a, b, th: 3.0 / b, "pp nn big"),
    ("a/(1+b^2)", lambda a, b, th: a / (1 + b ** 2), "pp np nn zero big"),
    ("(a-b)^2", lambda a, b, th: (a - b) ** 2, "pp np nn zero big"),
    ("a*a", lambda a, b, th: a * a, "pp np zero big"),                  # the same variable on both sides: the VSEL diagonal
    ("a*b*a", lambda a, b, th: a * b * a, "pp np nn zero big"),
    ("tanh(a*b)", lambda a, b, th: Unary("tanh", a * b), "pp np nn zero edge"),   # big: 1/cosh² is subnormal, then 0
    ("asin(a*b)", lambda a, b, th: Unary("asin", a * b), "zero edge"),
    ("a^theta", lambda a, b, th: a ** th, "pp np big"),                 # θ₀ = -1 is infinite, θ₀ in {0, 1} NaN at a = 0
)
FORMS = tuple(f[0] for f in BINARY_FORMS)


def binary_sweep():
    """Variables: ``a`` of form k at 2k·N, its ``b`` at (2k + 1)·N.  Row of form k: k·N + i.  One parameter θ₀."""
    core = ExaCore()
    ds, it = DataSource(), _items()
    th = core.add_par(np.array([THETAS[0]]))
    for _, make, _ in BINARY_FORMS:
        a, b = core.add_var(N, start=0.5), core.add_var(N, start=1.5)
        core.add_con(make(a[ds.i], b[ds.i], th[1]), it)
    core.theta_par = th
    return core


BUILDERS = {"unary_sweep": unary_sweep, "binary_sweep": binary_sweep}


def build_core(name):
    return BUILDERS[name]()


# ---- regions ---------------------------------------------------------------------------------------------------------------
def _lin(lo, hi, s=1.0):
    return lambda r, m: s * r.uniform(lo, hi, m)


def _geo(lo, hi):
    return lambda r, m: 10.0 ** r.uniform(math.log10(lo), math.log10(hi), m)


def _log(lo, hi, s=1.0):
    g = _geo(lo, hi)
    return lambda r, m: s * g(r, m)


def _near_one(lo, hi, s):       # 1 - |x| in geomspace(lo, hi)
    g = _geo(lo, hi)
    return lambda r, m: s * (1.0 - g(r, m))


def _past_one(lo, hi, s):       # |x| - 1 in geomspace(lo, hi)
    g = _geo(lo, hi)
    return lambda r, m: s * (1.0 + g(r, m))


EXPH = ("exp", "exp2", "sinh", "cosh", "tanh", "csch", "sech", "coth")
TRIG = ("sin", "cos", "tan", "csc", "sec", "cot")
DEG = ("sind", "cosd", "tand", "cscd", "secd", "cotd")
POSITIVE = ("sqrt", "log", "log2", "log10")      # domain x > 0 (sqrt: f' is infinite at 0)
UNIT = ("asin", "acos", "atanh")                 # domain |x| < 1 for all of f, f', f''


def unary_regions(op):
    """name -> draw(rng, count) of the regions of `op`, in tiling order."""
    if op == "acoth":
        return {"large+": _log(10, 1e8), "large-": _log(10, 1e8, -1.0),
                "edge+": _past_one(1e-6, 1e-2, 1.0), "edge-": _past_one(1e-6, 1e-2, -1.0)}
    neg = op not in POSITIVE
    reg = {"pos": _lin(0.3, 0.8)}
    if neg:
        reg["neg"] = _lin(0.3, 0.8, -1.0)
    tiny = (1e-14, 1e-3) if op == "log1p" else (1e-10, 1e-3)
    reg["tiny+"] = _log(*tiny)
    if neg:
        reg["tiny-"] = _log(*tiny, -1.0)
    if op in UNIT:
        reg["edge+"] = _near_one(1e-10, 1e-2, 1.0)
        reg["edge-"] = _near_one(1e-10, 1e-2, -1.0)
        return reg
    if op in EXPH:
        large = (_lin(5, 30), _lin(5, 30, -1.0))
    elif op in TRIG:
        large = (_lin(10.1, 200.3), _lin(10.1, 200.3, -1.0))
    elif op in DEG:
        large = (_lin(100.3, 719.7), _lin(100.3, 719.7, -1.0))
    else:
        large = (_log(10, 1e8), _log(10, 1e8, -1.0))
    reg["large+"] = large[0]
    if neg and op != "log1p":
        reg["large-"] = large[1]
    if op in TRIG:
        reg["huge"] = _log(1e5, 1e15)
    if op == "log1p":
        g = _geo(1e-8, 1e-2)
        reg["edge"] = lambda r, m: -1.0 + g(r, m)
    return reg


def _edge_pair(r, m):
    """a·b = 1 - δ EXACTLY, δ near geomspace(1e-9, 1e-3): `a` has 6 significant bits and `b` is cut to 40, so the product
    the kernel forms is the product the reference sees — the sweep is about the operator at 1 - δ, not about the rounding of
    a·b, which at δ = 1e-9 alone moves f'' by 1e-7."""
    a = r.integers(33, 64, m) / 64.0
    b = (1.0 - _geo(1e-9, 1e-3)(r, m)) / a
    mant, ex = np.frexp(b)
    return a, np.ldexp(np.round(mant * 2.0 ** 40) / 2.0 ** 40, ex)


BINARY_REGIONS = {
    "pp": lambda r, m: (r.uniform(0.3, 0.8, m), r.uniform(1.3, 1.9, m)),
    "np": lambda r, m: (-r.uniform(0.3, 0.8, m), r.uniform(1.3, 1.9, m)),
    "nn": lambda r, m: (-r.uniform(0.3, 0.8, m), -r.uniform(1.3, 1.9, m)),
    "zero": lambda r, m: (np.zeros(m), r.uniform(1.3, 1.9, m)),
    "big": lambda r, m: (_geo(10, 1e4)(r, m), r.uniform(5, 9, m)),
    "edge": _edge_pair,
}


def _tiling(names):
    """item -> region name, the regions tiled cyclically"""
    return [names[i % len(names)] for i in range(N)]


def region_names(model):
    """One list of N region names per slab-owning operator / form."""
    if model == "unary_sweep":
        return {op: _tiling(list(unary_regions(op))) for op in OPS}
    return {f: _tiling(regs.split()) for f, _, regs in BINARY_FORMS}


def points(model, seed):
    """The evaluation point of `model` ("unary_sweep" / "binary_sweep")."""
    rng = np.random.default_rng(seed)
    if model == "unary_sweep":
        x = np.empty((len(OPS) + 1) * N)
        for k, op in enumerate(OPS):
            regs = unary_regions(op)
            tile = np.array(_tiling(list(regs)))
            for name, draw in regs.items():
                sel = np.flatnonzero(tile == name)
                x[k * N + sel] = draw(rng, sel.size)
        x[len(OPS) * N:] = rng.uniform(1.3, 1.9, N)
        return x
    x = np.empty(2 * len(BINARY_FORMS) * N)
    for k, (_, _, regs) in enumerate(BINARY_FORMS):
        tile = np.array(_tiling(regs.split()))
        for name in regs.split():
            sel = np.flatnonzero(tile == name)
            a, b = BINARY_REGIONS[name](rng, sel.size)
            x[2 * k * N + sel], x[(2 * k + 1) * N + sel] = a, b
    return x


# ---- who an output element belongs to -----------------------------------------------------------------------------------------
def owner_of_col(model, col):
    """(operator or form, item) of a variable; the unary model's shared slab is ("b", item)."""
    k, i = divmod(int(col), N)
    if model == "unary_sweep":
        return (OPS[k] if k < len(OPS) else "b"), i
    return FORMS[k // 2], i


def owner_of_row(model, row):
    k, i = divmod(int(row), N)
    if model == "unary_sweep":
        return OPS[k % len(OPS)], i
    return FORMS[k], i


def templates_of(model, name):
    """template indices that read the slab(s) of operator / form `name`"""
    if model == "unary_sweep":
        k = OPS.index(name)
        return [k, len(OPS) + k, 2 * len(OPS) + k]
    return [FORMS.index(name)]


# ---- special points ------------------------------------------------------------------------------------------------------------
LN2 = 0.6931471805599453
# operator -> [(x, (f, f', f'') where the limit is finite and the table returns it EXACTLY, else None)]; None alone: only the
# class (NaN, +inf, -inf, finite) of every element is pinned, to the oracle's
_Z = (0.0, -0.0)
SPECIAL_UNARY = {
    "abs": [(z, (0.0, 1.0, 0.0)) for z in _Z],          # the rule x >= 0: f' = 1 at -0.0 too
    "abs2": [(z, (0.0, 0.0, 2.0)) for z in _Z],
    "sin": [(z, (0.0, 1.0, 0.0)) for z in _Z],
    "tan": [(z, (0.0, 1.0, 0.0)) for z in _Z],
    "atan": [(z, (0.0, 1.0, 0.0)) for z in _Z],
    "asin": [(z, (0.0, 1.0, 0.0)) for z in _Z] + [(1.0, None), (-1.0, None)],
    "sinh": [(z, (0.0, 1.0, 0.0)) for z in _Z],
    "tanh": [(z, (0.0, 1.0, 0.0)) for z in _Z],
    "cbrt": [(z, None) for z in _Z],
    "log1p": [(z, (0.0, 1.0, -1.0)) for z in _Z],
    "exp": [(z, (1.0, 1.0, 1.0)) for z in _Z],
    "exp2": [(z, (1.0, LN2, LN2 * LN2)) for z in _Z],
    "cos": [(z, (1.0, 0.0, -1.0)) for z in _Z],
    "cosh": [(z, (1.0, 0.0, 1.0)) for z in _Z],
    "sec": [(z, (1.0, 0.0, 1.0)) for z in _Z],
    "sech": [(z, (1.0, 0.0, -1.0)) for z in _Z],
    "sqrt": [(0.0, None)],
    "log": [(1.0, (0.0, 1.0, -1.0))],
    "acos": [(1.0, None), (-1.0, None)],
    "atanh": [(1.0, None), (-1.0, None)],
    "acot": [(0.0, (None, -1.0, 0.0)), (-0.0, (None, -1.0, 0.0))],      # f = ±π/2: left to the class check and the oracle
}
# the constant-exponent forms at a = 0
SPECIAL_BINARY = {
    "a^2": (0.0, 0.0, 2.0), "a^3": (0.0, 0.0, 0.0), "a^1": (0.0, 1.0, 0.0), "a^0": (1.0, 0.0, 0.0), "a^2.5": (0.0, 0.0, 0.0),
    "a^-2": None, "a^0.5": None,
}


def special_points(model):
    """A small exact second point: the special arguments at the first items of their slab, an in-domain constant elsewhere."""
    if model == "unary_sweep":
        x = np.full((len(OPS) + 1) * N, 0.5)
        x[OPS.index("acoth") * N:(OPS.index("acoth") + 1) * N] = 2.0
        x[len(OPS) * N:] = 1.5
        for op, pts in SPECIAL_UNARY.items():
            for j, (v, _) in enumerate(pts):
                x[OPS.index(op) * N + j] = v
        return x
    x = np.tile(np.concatenate([np.full(N, 0.5), np.full(N, 1.5)]), len(BINARY_FORMS))
    for f in list(SPECIAL_BINARY) + ["a^theta"]:
        k = FORMS.index(f)
        x[2 * k * N:(2 * k + 1) * N] = 0.0
    k = FORMS.index("asin(a*b)")
    x[(2 * k + 1) * N:(2 * k + 2) * N] = 1.25      # a·b = 0.625
    return x
