"""Higher-order derivatives on the host interface: `deriv(q, x, x)` nests first-order derivatives, one variable slab and
one set of approximation rows per level — what `reformulate_high_order_derivatives!` leaves behind
(/root/reference/src/transform.jl:141-142), with `derivative_expr_data` called per level (transform.jl:535)."""
import numpy as np

from infiniteexamodels.jl_amd import transcribe
from infiniteexamodels.jl_amd.core import T_CON
from infiniteexamodels.jl_amd.infinite import FiniteDifference, InfiniteModel
from pyoracle import OracleModel


def test_second_derivative_mapping_and_count(built):
    """/root/reference/test/transcription.jl:19-20 (`d1 = deriv(y, t)`, `d2 = deriv(q, x, x)`) and :58-62 (the mapping of
    d2 is a 5 x 5 slab, `num_derivatives(m) == 3`): the lines tests/test_transcription.py::test_mapping_initializers left out."""
    m = InfiniteModel()
    t = m.infinite_parameter("t", 0.0, 1.0, num_supports=5)
    x = m.infinite_parameter("x", -1.0, 1.0, num_supports=5)
    y = m.variable("y", t)
    q = m.variable("q", t, x)
    d1 = m.deriv(y, t)
    d2 = m.deriv(q, x, x)
    assert d2.arg is m.deriv(q, x) and d2.pref is x and d2.arg.arg is q          # one first-order derivative per level
    assert m.deriv(q, x, x) is d2 and m.deriv(m.deriv(q, x), x) is d2 and m.deriv(y, t) is d1
    assert len(m.derivatives) == 3                                               # :62
    m.constraint(d1 + y == 0)
    m.constraint(d2 - q == 0)
    m.objective("min", m.integral(y ** 2, t))
    data = transcribe.ExaMappingData()
    core = transcribe.exa_core(m, data)
    assert data.infvar_mappings[d2].length == 25 and tuple(data.infvar_mappings[d2].size) == (5, 5)   # :58-61
    assert data.infvar_mappings[d2.arg].length == 25
    rows = [tp for tp in core.templates if tp.kind == T_CON and tp.tag and tp.tag[0] == "deriv"]
    assert [len(tp.items) for tp in rows] == [4, 20, 20]                         # backward rows of y; of ∂q/∂x; of ∂²q/∂x²
    # a mixed derivative comes for free: another level on the other parameter
    d3 = m.deriv(q, t, x)
    assert d3.pref is x and d3.arg is m.deriv(q, t) and len(m.derivatives) == 5


def test_nested_central_differences_of_x_squared(built):
    """y = x² on a uniform grid, central differences on both levels: the transcribed rows `(x[i+1] − x[i−1])·d[i] − v[i+1] +
    v[i−1] = 0` (the `d_arg` coefficient of `derivative_expr_data`, transform.jl:535-557) hold for the exact nested values —
    d1 = 2x, d2 = 2.  All data are dyadic rationals, so the rows are satisfied to rounding: rtol 1e-12 on O(1) numbers."""
    n, h = 9, 0.25
    m = InfiniteModel()
    x = m.infinite_parameter("x", 0.0, (n - 1) * h, num_supports=n, derivative_method=FiniteDifference("central"))
    y = m.variable("y", x)
    d2 = m.deriv(y, x, x)
    d1 = d2.arg
    m.constraint(d2 - 2 == 0)
    m.objective("min", m.integral(y ** 2, x))
    data = transcribe.ExaMappingData()
    core = transcribe.exa_core(m, data)
    om = OracleModel(core.to_blob())
    s = np.arange(n) * h
    xv = np.zeros(om.nvar)
    off = lambda v: data.infvar_mappings[v].offset
    xv[off(y):off(y) + n] = s ** 2
    # level 1 has rows on 1..n-2 only, where the central difference of x² is exact; its two end values have no row and
    # are set to 2x as well, which is what the level-2 rows next to them need
    xv[off(d1):off(d1) + n] = 2 * s
    xv[off(d2):off(d2) + n] = 2.0
    c = om.cons(xv)
    rows = {tp.tag[1]: tp for tp in core.templates if tp.kind == T_CON and tp.tag and tp.tag[0] == "deriv"}
    assert sorted(len(tp.items) for tp in rows.values()) == [n - 2, n - 2]
    for tp in rows.values():
        np.testing.assert_allclose(1.0 + c[tp.o0:tp.o0 + len(tp.items)], 1.0, rtol=1e-12)
        np.testing.assert_array_equal(tp.items.column("d_arg1"), np.full(n - 2, 2 * h))
    # a wrong second derivative is seen by exactly the level-2 rows: residual (x[i+1] − x[i−1])·δ
    xv[off(d2):off(d2) + n] = 2.5
    c2 = om.cons(xv)
    t2 = rows[max(rows)]
    np.testing.assert_allclose(c2[t2.o0:t2.o0 + n - 2], np.full(n - 2, 2 * h * 0.5), rtol=1e-12)
