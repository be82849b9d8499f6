"""Models with stencils that reach to the RIGHT of their support — forward and central finite differences
(/root/reference/src/transform.jl:535 hands any finite-difference method to `derivative_expr_data`) — and the
heat-equation workload with its nested second derivative (transform.jl:141, test/transcription.jl:20).  Shared by the
CPU and GPU tests of the two-sided stencils; cases.py stays the list of the models that existed before."""
import numpy as np

from infiniteexamodels.jl_amd import transcribe, workloads
from infiniteexamodels.jl_amd.infinite import FiniteDifference, InfiniteModel, sin


def ode_1d_supports(n: int = 23) -> np.ndarray:
    return np.linspace(0.0, 2.0, n) ** 1.3


def ode_1d(method: str, n: int = 23, supports=None) -> InfiniteModel:
    """A 1-D optimal-control model on a non-uniform grid: nonlinear dynamics, a second state whose derivative row is
    linear, a point constraint and a tracking objective."""
    m = InfiniteModel()
    s = ode_1d_supports(n) if supports is None else supports   # (an explicit window: the Python shard path, shard.window)
    t = m.infinite_parameter("t", 0.0, float(s[-1]), supports=s, derivative_method=FiniteDifference(method))
    y = m.variable("y", t, start=1.0)
    z = m.variable("z", t, start=0.5)
    u = m.variable("u", t, lb=-2.0, ub=2.0, start=0.1)
    w = m.variable("w", lb=0.0, start=0.3)
    m.constraint(m.deriv(y, t) == -y * u + sin(z) * w)
    m.constraint(m.deriv(z, t) == y - z)
    m.constraint(y(0) == 1)
    m.objective("min", m.integral((y - 0.5) ** 2 + 0.1 * u ** 2 + z ** 2, t) + w ** 2)
    return m


MODELS = {
    "forward_1d": lambda: ode_1d("forward"),
    "central_1d": lambda: ode_1d("central"),
    "heat_central": lambda: workloads.heat(7, 9, "central"),
    "heat_forward": lambda: workloads.heat(6, 8, "forward"),
}


# the sizes the multi-process GPU test shards (tests/comm_worker_two_sided.py; pre-compiled by the build)
COMM_MODELS = {
    "central_1d": lambda: ode_1d("central", 3001), "forward_1d": lambda: ode_1d("forward", 3000),
    "heat_central": lambda: workloads.heat(40, 61, "central"), "heat_forward": lambda: workloads.heat(30, 50, "forward"),
}


def build_core(name: str):
    return transcribe.exa_core(MODELS[name]())


def eval_point(om, seed: int = 0):
    x = om.x0 + 0.1 * np.random.default_rng(seed).standard_normal(om.nvar)
    y = np.random.default_rng(seed + 1).standard_normal(om.ncon)
    return x, y
