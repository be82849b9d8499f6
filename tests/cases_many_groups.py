"""Models over more than three infinite-parameter groups: their item products fold into a box of at
most three runs (infiniteexamodels.jl_amd/items.py: fold_runs)."""
from __future__ import annotations

import numpy as np

from infiniteexamodels.jl_amd import infinite as io
from infiniteexamodels.jl_amd import transcribe
from infiniteexamodels.jl_amd.infinite import InfiniteModel


def four_groups(nt=6, nx=4, na=3, nb=5):
    """y(t, x, a, b) with ∂(y, t) == -a·y + u(t) + … : a space-time model with two uncertain
    parameters.  Variables over all four groups and over subsets (u(t), q(x, t), w(b)), backward
    differences along a fast axis (t) and a slow one (b), an initial condition (a semi-infinite
    variable), a measure over one parameter and nonlinear terms."""
    m = InfiniteModel()
    t = m.infinite_parameter("t", 0, 1, num_supports=nt)
    x = m.infinite_parameter("x", -1, 1, num_supports=nx)
    a = m.infinite_parameter("a", 0.5, 1.5, num_supports=na)
    b = m.infinite_parameter("b", 0, 2, num_supports=nb)
    y = m.variable("y", t, x, a, b, start=0.5)
    u = m.variable("u", t, lb=-2, ub=2, start=0.1)
    q = m.variable("q", x, t, start=0.2)
    w = m.variable("w", b, start=0.3)
    z = m.variable("z", start=1.0)
    m.constraint(m.deriv(y, t) == -a * y + u + 0.1 * io.sin(q) * w)
    m.constraint(m.deriv(y, b) == io.exp(-y) * w - x * y * z)
    m.constraint(y(0, x, a, b) == 1)
    m.constraint(m.deriv(q, t) == u * q - x)
    m.constraint(y * w + a * q <= 3 + b)
    m.objective("min", m.integral(u ** 2, t) + z ** 2
                + m.integral(m.integral(m.integral(m.integral(y ** 2, t), x), a), b))
    return m


def five_groups(nt=4, nx=3, na=2, nb=3, nc=3):
    """y(t, x, a, b, c): a derivative along x (the second axis), a parameter of a merged run inside
    the dynamics, a variable over the slowest group only and a measure over c."""
    m = InfiniteModel()
    t = m.infinite_parameter("t", 0, 1, num_supports=nt)
    x = m.infinite_parameter("x", -1, 1, num_supports=nx)
    a = m.infinite_parameter("a", 0.5, 1.5, num_supports=na)
    b = m.infinite_parameter("b", 0, 1, num_supports=nb)
    c = m.infinite_parameter("c", 1, 2, num_supports=nc)
    y = m.variable("y", t, x, a, b, c, start=0.4)
    v = m.variable("v", c, start=0.2)
    r = m.variable("r", a, b, start=0.1)
    m.constraint(m.deriv(y, x) == -b * y + io.cos(v) * r - t)
    m.constraint(m.deriv(y, c) == y * v * a)
    m.constraint(y(t, 0, a, b, c) == 0.5 + t)
    m.objective("min", m.integral(v ** 2, c)
                + m.integral(m.integral(m.integral(m.integral(m.integral(io.exp(0.1 * y), t), x), a), b), c))
    return m


def many_group_cases():
    """name -> model builder (small models: every test over them)."""
    return {
        "four_groups": four_groups,
        "four_groups_b": lambda: four_groups(5, 3, 4, 3),
        "five_groups": five_groups,
    }


def large_four_groups():
    """The 4-group model at about 2·10⁵ items per template."""
    return four_groups(100, 20, 10, 10)


def build_core(name):
    if name == "large_four_groups":
        return transcribe.exa_core(large_four_groups())
    return transcribe.exa_core(many_group_cases()[name]())


def eval_point(om, seed=0):
    rng = np.random.default_rng(seed)
    x = np.abs(om.x0 + 0.1 * rng.standard_normal(om.nvar)) + 0.05
    y = np.random.default_rng(seed + 1).standard_normal(om.ncon)
    return x, y
