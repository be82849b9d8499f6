"""Hand-built degenerate models for the scaled solver phases: no constraint at all (and a block of variables nothing reads),
no objective at all, and a linear program (no second-order slot: the accepted phase has no Hessian member)."""
import numpy as np

from infiniteexamodels.jl_amd.core import ExaCore
from infiniteexamodels.jl_amd.items import Items
from infiniteexamodels.jl_amd.nodes import DataSource


def unconstrained(n=70):
    core, ds = ExaCore(), DataSource()
    y = core.add_var(n, start=1.0 + 0.01 * np.arange(n))
    core.add_var(5, start=0.5)      # untouched
    core.add_obj((y[ds.i] - 1.0) ** 3 * (1.0 + ds.t), Items.from_supports("i", n, {"t": np.linspace(0.0, 1.0, n)}, group_id=1))
    return core


def no_objective(n=90):
    core, ds = ExaCore(), DataSource()
    y = core.add_var(n, start=1.0 + 0.01 * np.arange(n))
    core.add_con(y[ds.i] ** 2 * (1.0 + ds.t) - 1.0, Items.from_supports("i", n, {"t": np.linspace(0.0, 1.0, n)}, group_id=1))
    return core


def linear(n=600):
    core, ds = ExaCore(), DataSource()
    y = core.add_var(n, start=1.0)
    sup = np.linspace(0.0, 1.0, n)
    g = Items.from_supports("i", n, {"t": sup}, group_id=1)
    # (a product with item data has no second-order slot; a quotient would have structural ones)
    core.add_con((y[ds.i] - y[ds.i - 1]) * ds.h - 2.0 * y[ds.i], g.select(1, n - 1).with_float("h", 1.0 / np.diff(sup)))
    core.add_con(y[1] * 3.0)
    core.add_obj(y[ds.i] * ds.t, g)
    return core


DEGENERATE = {"unconstrained": unconstrained, "no_objective": no_objective, "linear": linear}
