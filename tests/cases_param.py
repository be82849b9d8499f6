"""Models for the parameter sensitivities (jpprod / jptprod / hpprod): every shape in which θ is read.

  * the models of cases.py with parameters (finite parameters shared by all items: rosenbrock; parameter functions
    read once per support: quadrotor, its collocation variant, pfun, pfun_full) and the heat workload;
  * ``shifted_pf``: a parameter function read THROUGH A STENCIL SHIFT (θ[i-1], θ[i], θ[i+1] from the row at i — what the
    modelling layer never writes, a hand-built core does) next to a finite parameter every item reads;
  * ``four_groups_param``: the folded four-group model of cases_many_groups.py with a finite parameter and a
    parameter function of t inside the folded rows."""
import numpy as np

import cases
import cases_two_sided
from infiniteexamodels.jl_amd import infinite as io
from infiniteexamodels.jl_amd import transcribe
from infiniteexamodels.jl_amd.core import ExaCore
from infiniteexamodels.jl_amd.infinite import InfiniteModel
from infiniteexamodels.jl_amd.items import Items
from infiniteexamodels.jl_amd.nodes import FUNCS, DataSource


def shifted_pf(n=150):
    rng = np.random.default_rng(11)
    core = ExaCore()
    y = core.add_var(n, start=1.0 + 0.1 * rng.standard_normal(n))
    u = core.add_var(n, start=0.1)
    pf = core.add_par(np.sin(np.linspace(0.0, 3.0, n)) + 1.5)
    k = core.add_par(np.array([0.7]))
    ds = DataSource()
    sup = np.linspace(0.0, 1.0, n)
    g = Items.from_supports("i", n, {"t": sup}, group_id=1)
    back = g.select(1, n - 1).with_float("h", np.diff(sup))            # i = 2..n
    inner = g.select(1, n - 2)                                         # i = 2..n-1
    core.add_con((y[ds.i] - y[ds.i - 1]) / ds.h - k[1] * (pf[ds.i - 1] * y[ds.i - 1] + FUNCS["sin"](pf[ds.i]) * u[ds.i]), back)
    core.add_con(u[ds.i] * pf[ds.i + 1] - FUNCS["exp"](pf[ds.i - 1] * y[ds.i]) * k[1] + pf[ds.i] ** 2, inner, lcon=-np.inf, ucon=5.0)
    core.add_con(y[1] - pf[1])
    core.add_obj((y[ds.i] - pf[ds.i]) ** 2 + k[1] * u[ds.i] ** 2 * ds.t, g)
    core.add_obj(k[1] ** 2 * y[n])
    return core


def four_groups_param(nt=6, nx=4, na=3, nb=5):
    m = InfiniteModel()
    t = m.infinite_parameter("t", 0, 1, num_supports=nt)
    x = m.infinite_parameter("x", -1, 1, num_supports=nx)
    a = m.infinite_parameter("a", 0.5, 1.5, num_supports=na)
    b = m.infinite_parameter("b", 0, 2, num_supports=nb)
    kap = m.finite_parameter("kap", 0.8)
    pf = m.parameter_function("pf", lambda s: 1.0 + np.cos(2.0 * s), t)
    y = m.variable("y", t, x, a, b, start=0.5)
    u = m.variable("u", t, lb=-2, ub=2, start=0.1)
    w = m.variable("w", b, start=0.3)
    m.constraint(m.deriv(y, t) == -a * kap * y + u * pf + 0.1 * io.sin(pf * y) * w)
    m.constraint(m.deriv(y, b) == io.exp(-y) * w - x * y * kap)
    m.constraint(y(0, x, a, b) == 1)
    m.constraint(y * w * pf <= 3 + b)
    m.objective("min", m.integral(kap * u ** 2 + pf * u, t)
                + m.integral(m.integral(m.integral(m.integral(y ** 2, t), x), a), b))
    return m


BUILDERS = {
    "shifted_pf": shifted_pf,
    "shifted_pf_3000": lambda: shifted_pf(3000),      # several workgroups: block seams of the pulled neighbours, the cross-workgroup reduction
    "four_groups_param": lambda: transcribe.exa_core(four_groups_param(), transcribe.ExaMappingData()),
}
# every model of cases.py with npar > 0, the heat workload, and the ones above
CASES_PY = ["quadrotor_1", "quadrotor_5", "quadrotor_100", "quadrotor_1000", "quadrotor_oc3_40", "quadrotor_oc3_700", "pfun_full", "rosenbrock", "pfun"]
HEAT = ["heat_central", "heat_forward"]
NAMES = CASES_PY + HEAT + list(BUILDERS)
# no parameter at all: the kinds write zeros / launch nothing
NO_PARAM = ["pandemic_20x3", "farmer_5"]


def build_core(name):
    if name in BUILDERS:
        return BUILDERS[name]()
    if name in cases_two_sided.MODELS:
        return cases_two_sided.build_core(name)
    return cases.build_core(name)


def eval_point(name, om, seed=0):
    if name in cases.small_cases():
        return cases.eval_point_for(name, om, seed)
    x = om.x0 + 0.1 * np.random.default_rng(seed).standard_normal(om.nvar)
    y = np.random.default_rng(seed + 1).standard_normal(om.ncon)
    return x, y
