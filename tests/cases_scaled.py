"""A hand-built model for the scaled program (rowmax / cons_scaled / jac_scaled): rows without any first-order slot, and a
row that is NaN at a chosen point.

  * ``log(y[i])·u[i]`` and ``u[i]·log(y[i])`` over the grid: at a point with ONE negative ``y`` the value of those two rows
    and their entry ``∂/∂u = log(y)`` are NaN (``∂/∂y = u/y`` is finite: a bare ``log(y[i])`` row would have a finite
    Jacobian) — the NaN slot comes second in the first row and first in the second, so a maximum that drops a NaN on
    either side is caught; the row maximum and both scaled outputs must carry the NaN in those rows and nowhere else;
  * ``2·t_i`` over the grid: item data only, no slot — its row maximum is 0.0 with the sign bit clear, its scaled value
    ``s·2·t_i``;
  * a product row ``y[i]·u[i] − t_i`` and a difference row, so that the grid has computed rows and data rows (both bodies
    of a split jac_coord!);
  * a scalar constraint without a variable."""
import numpy as np

from infiniteexamodels.jl_amd.core import ExaCore
from infiniteexamodels.jl_amd.items import Items
from infiniteexamodels.jl_amd.nodes import FUNCS, DataSource

N = 700          # more than one workgroup in the lane-fused shape
NAN_ITEM = 333   # 0-based item whose y is negative at nan_point()


def nan_and_constant_rows(n=N):
    core = ExaCore()
    y = core.add_var(n, start=1.0 + 0.001 * np.arange(n))
    u = core.add_var(n, start=0.5)
    ds = DataSource()
    sup = np.linspace(0.0, 1.0, n)
    g = Items.from_supports("i", n, {"t": sup}, group_id=1)
    back = g.select(1, n - 1).with_float("h", np.diff(sup))
    core.add_con(FUNCS["log"](y[ds.i]) * u[ds.i], g)            # rows 0 .. n-1
    core.add_con(2.0 * ds.t + 0.25, g)                          # rows n .. 2n-1: no slot at all
    core.add_con(y[ds.i] * u[ds.i] - ds.t, g)                   # rows 2n .. 3n-1
    core.add_con((y[ds.i] - y[ds.i - 1]) / ds.h - u[ds.i], back)   # rows 3n .. 4n-2: partials are item data
    core.add_con(u[ds.i] * FUNCS["log"](y[ds.i]), g)            # rows 4n-1 .. 5n-2: the same slots in the other order
    core.add_obj((y[ds.i] - 1.0) ** 2 + u[ds.i] ** 2 * ds.t, g)
    return core


def nan_point(om, seed=0):
    """a point whose only negative y sits at item NAN_ITEM"""
    rng = np.random.default_rng(seed)
    x = np.asarray(om.x0, dtype=np.float64) + 0.05 * rng.random(om.nvar)
    x[NAN_ITEM] = -0.7
    return x


def rows_of(n=N):
    """(the NaN rows, the rows without a slot)"""
    return np.array([NAN_ITEM, 4 * n - 1 + NAN_ITEM]), np.arange(n, 2 * n)
