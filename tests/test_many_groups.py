"""Models over more than three infinite-parameter groups (the reference's Iterators.product over any
number of item iterators, transform.jl:443-445): the producer folds the product into a box of at
most three runs without changing the wire format, so the frozen oracle evaluates the very bytes the
generated kernels run.  CPU only."""
import copy
import hashlib
import itertools
import json
import os
import warnings

import numpy as np
import pytest

import cases
import cases_many_groups as MG
from emu import EmulatedModel
from infiniteexamodels.jl_amd import lib as iemlib
from infiniteexamodels.jl_amd import transcribe
from infiniteexamodels.jl_amd.items import Field, Items, fold_runs
from pyoracle import OracleModel

NAMES = list(MG.many_group_cases())


def _core(name):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = MG.many_group_cases()[name]()
        data = transcribe.ExaMappingData()
        return transcribe.exa_core(m, data), data, m


def _rel(a, b):
    if len(b) == 0:
        return 0.0
    return float(np.abs(a - b).max() / max(1e-300, np.abs(b).max()))


# 1 -- transcription -----------------------------------------------------------------------------
def test_product_of_four_factors_is_julia_order():
    f = [Items.from_supports(f"group_idx{g}", n, {f"ip{g}": np.linspace(0, 1, n) + g}, group_id=g)
         for g, n in zip((1, 2, 3, 4), (3, 2, 4, 2))]
    p = f[0].product(f[1]).product(f[2]).product(f[3])
    want = [{**r0, **r1, **r2, **r3} for r3, r2, r1, r0 in itertools.product(*[x.records() for x in reversed(f)])]
    assert p.records() == want
    folded = p.fold(fold_runs(p.dims, p.free))
    assert len(folded.dims) == 3 and folded.records() == want


def test_fold_rule():
    assert fold_runs((2, 3, 4, 5), (True,) * 4) == [(0, 1), (1, 2), (2, 4)]
    assert fold_runs((2, 3, 4, 5), (False, True, True, True)) == [(0, 1), (1, 2), (2, 4)]
    assert fold_runs((2, 3, 4, 5), (True, True, True, False)) == [(0, 1), (1, 2), (2, 4)]     # restricted axis ends its run
    assert fold_runs((2, 3, 4, 5), (True, True, False, True)) == [(0, 1), (1, 3), (3, 4)]
    assert fold_runs((2, 3, 4, 5, 6, 7), (True, True, True, False, True, True)) == [(0, 1), (1, 4), (4, 6)]
    with pytest.raises(ValueError, match="cannot fold"):
        fold_runs((2, 3, 4, 5, 6), (False, False, False, True, True))


@pytest.mark.parametrize("name", NAMES)
def test_templates_enumerate_the_reference_product(name):
    core, data, m = _core(name)
    folded = [t for t in core.templates if t.items.grid is not None and any(g >= 3500 for g in t.items.grid[0])]
    assert folded, "the model must exercise the fold"
    checked = 0
    for t in core.templates:
        kind, i = t.tag[0], t.tag[1]
        if kind == "con":
            groups = transcribe.parameter_group_int_indices(m.constraints[i].func)
            if len(groups) < 4:
                continue
            factors = [data.base_itrs[g - 1] for g in groups]
        elif kind == "deriv":
            d = m.derivatives[i]
            groups = d.arg.group_idxs
            if len(groups) < 4:
                continue
            base = data.base_itrs[d.pref.group.index - 1]
            idxs, cols = transcribe.derivative_expr_data(d.pref.group.derivative_method, base.column(data.param_alias[d.pref]))
            pref_itr = base.take(idxs).with_float("d_arg1", cols[0])
            factors = [pref_itr if g == d.pref.group.index else data.base_itrs[g - 1] for g in groups]
        else:
            continue
        want = []
        for rs in itertools.product(*[f.records() for f in reversed(factors)]):
            rec = {}
            for r in reversed(rs):
                rec.update(r)
            want.append(rec)
        assert len(t.items.dims) <= 3
        assert t.items.records() == want, t.tag
        checked += 1
    assert checked >= 3


@pytest.mark.parametrize("name", NAMES)
def test_blob_stays_within_the_format(name):
    core, _, _ = _core(name)
    for t in core.templates:
        assert 1 <= len(t.items.dims) <= 3
        assert all(len(f.steps) == len(t.items.dims) for f in t.ifields + t.ffields)
        assert all(len(terms) <= 3 for _, terms in t.idx)
        for f in t.ifields:   # a digit / run column is never item-length on a merged box
            if f.mode == "gather" and len(t.items) > 1:
                assert len(f.arr) < len(t.items)
    for off, dims, groups in core.slabs:
        assert 1 <= len(dims) <= 3 and len(groups) == len(dims)
    om = OracleModel(core.to_blob())
    assert om.nvar == core.nvar and om.ncon == core.ncon


def test_unfoldable_index_is_refused():
    """Every run contributes at most one index term, but an explicit integer column over two runs needs
    one of its own: with all three runs in use that is a fourth — refused, never a corrupt blob."""
    core, _, _ = _core("four_groups")
    dims = (3, 2, 2, 2)
    fields = {f"g{d + 1}": Field("int", "affine", 1, tuple(int(e == d) for e in range(4))) for d in range(4)}
    fields["h"] = Field("int", "gather", 0, (1, 3, 0, 0), np.array([1, 3, 2, 1, 2, 3], dtype=np.int64))
    p = Items(dims, fields, free=(True,) * 4)
    from infiniteexamodels.jl_amd import nodes as N
    ds = N.DataSource()
    v = core.add_var(3, 2, 2, 2)
    core.add_con(v[ds["h"], ds["g2"], ds["g3"], ds["g4"]], p)            # h over runs (0), (1); run (2, 3): 3 terms
    with pytest.raises(ValueError, match="needs 4 item fields"):
        core.add_con(v[ds["g1"], ds["g2"], ds["g3"], ds["g4"]] + v[ds["h"], ds["g2"], 1, 1] * v[ds["h"], 1, ds["g3"], 1]
                     + v[ds["h"] + ds["g1"], ds["g2"], ds["g3"], ds["g4"]], p)


# 2 -- two encodings -----------------------------------------------------------------------------
def _explicit_template(t):
    """Same template over a 1-D explicit list: every field as an item-length column."""
    u = copy.copy(t)
    dims = t.items.dims
    u.ifields = [Field("int", "gather", 0, (1,), np.ascontiguousarray(f.values(dims), dtype=np.int64)) for f in t.ifields]
    u.ffields = [Field("float", "gather", 0, (1,), np.ascontiguousarray(f.values(dims), dtype=np.float64)) for f in t.ffields]
    u.items = Items((len(t.items),), {})
    return u


def explicit_blob(core):
    c = copy.copy(core)
    c.templates = [_explicit_template(t) for t in core.templates]
    return c, c.to_blob()


@pytest.mark.parametrize("name", NAMES)
def test_folded_and_explicit_encodings_agree(name, built):
    core, _, _ = _core(name)
    a = OracleModel(core.to_blob())
    _, eb = explicit_blob(core)
    b = OracleModel(eb)
    assert (a.nvar, a.ncon, a.nnzj, a.nnzh) == (b.nvar, b.ncon, b.nnzj, b.nnzh)
    for fa, fb in ((a.jac_structure, b.jac_structure), (a.hess_structure, b.hess_structure)):
        ra, ca = fa()
        rb, cb = fb()
        assert np.array_equal(ra, rb) and np.array_equal(ca, cb)
    x, y = MG.eval_point(a)
    assert a.obj(x) == b.obj(x)
    for va, vb in ((a.cons(x), b.cons(x)), (a.grad(x), b.grad(x)), (a.jac_coord(x), b.jac_coord(x)),
                   (a.hess_coord(x, y, 0.7), b.hess_coord(x, y, 0.7))):
        assert va.tobytes() == vb.tobytes()


def test_four_groups_against_numpy():
    core, data, m = _core("four_groups")
    om = OracleModel(core.to_blob())
    x, _ = MG.eval_point(om)
    g = {p.name: m.groups[i].supports[:, 0] for i, p in enumerate(gr.prefs[0] for gr in m.groups)}
    nt, nx, na, nb = (len(g[k]) for k in "txab")
    vs = {v.name: v for v in m.infinite_variables}

    def val(name):
        s = data.infvar_mappings[vs[name]]
        return x[s.offset:s.offset + s.length].reshape(s.size, order="F")
    y, u, q, w = val("y"), val("u"), val("q"), val("w")
    z = x[data.finvar_mappings[m.finite_variables[0]].i - 1]
    dy = x[data.infvar_mappings[m.derivatives[0]].offset:][:y.size].reshape(y.shape, order="F")
    T, X, A, B = np.meshgrid(g["t"], g["x"], g["a"], g["b"], indexing="ij")
    # c0: ∂(y, t) == -a·y + u(t) + 0.1·sin(q(x, t))·w(b), written lhs - rhs over the full product
    want = dy - (-A * y + u[:, None, None, None] + 0.1 * np.sin(q.T[:, :, None, None]) * w[None, None, None, :])
    c0 = om.cons(x)[:y.size].reshape(y.shape, order="F")
    assert np.allclose(c0, want, rtol=1e-14, atol=1e-14)
    # objective: ∫u² dt + z² + ∫∫∫∫ y² (trapezoid weights)
    def trap(s):
        d = np.diff(s)
        c = np.zeros_like(s)
        c[:-1] += d / 2
        c[1:] += d / 2
        return c
    wt, wx, wa, wb = (trap(g[k]) for k in "txab")
    want_obj = np.dot(wt, u ** 2) + z ** 2 + np.einsum("i,j,k,l,ijkl->", wt, wx, wa, wb, y ** 2)
    assert abs(om.obj(x) - want_obj) <= 1e-12 * abs(want_obj)


# 3 -- generated kernels (emulated) ---------------------------------------------------------------
@pytest.mark.parametrize("digits", [1, 0])
@pytest.mark.parametrize("name", NAMES)
def test_emulated_kernels_match_oracle(name, digits, grid_mode):
    core, _, _ = _core(name)
    blob = core.to_blob()
    om = OracleModel(blob)
    x, y = MG.eval_point(om)
    with iemlib.options(digit_fields=digits):
        _emulate_and_compare(core, blob, om, x, y)


def _emulate_and_compare(core, blob, om, x, y):
    em = EmulatedModel(core, blob)
    assert abs(em.obj(x) - om.obj(x)) <= 1e-14 * max(1.0, abs(om.obj(x)))
    assert _rel(em.cons(x), om.cons(x)) <= 1e-14
    assert _rel(em.grad(x), om.grad(x)) <= 1e-14
    j = em.jac_coord(x, om.nnzj)
    h = em.hess_coord(x, y, 0.7, om.nnzh)
    assert not np.isnan(j).any() and not np.isnan(h).any()
    assert _rel(j, om.jac_coord(x)) <= 1e-14
    assert _rel(h, om.hess_coord(x, y, 0.7)) <= 1e-14
    jp, hp = em.jac_hess_coord(x, y, 0.7, om.nnzj, om.nnzh)
    assert np.array_equal(jp, j) and np.array_equal(hp, h)
    f, c = em.eval_trial(x)
    assert f == em.obj(x) and np.array_equal(c, em.cons(x))
    g, ja, ha = em.eval_accepted(x, y, 0.7, om.nnzj, om.nnzh)
    assert np.array_equal(g, em.grad(x)) and np.array_equal(ja, j) and np.array_equal(ha, h)
    rng = np.random.default_rng(5)
    v, vc = rng.standard_normal(om.nvar), rng.standard_normal(om.ncon)
    assert _rel(em.jprod(x, v), om.jprod(x, v)) <= 1e-13
    assert _rel(em.jtprod(x, vc), om.jtprod(x, vc)) <= 1e-13
    assert _rel(em.hprod(x, y, v, 0.7), om.hprod(x, y, v, 0.7)) <= 1e-13


# 4 -- the decode removes the reads --------------------------------------------------------------
def _plan_rbytes(blob, kind):
    return sum(int(line.split()[11]) for line in iemlib.emit_launch_plan(blob).splitlines()
               if line.startswith("kernel ") and int(line.split()[3]) == kind)


@pytest.mark.parametrize("name", NAMES + ["large_four_groups"])
def test_digit_decode_removes_column_reads(name, built):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        core = MG.build_core(name)
    blob = core.to_blob()
    digit_arrays = set()
    for t in core.templates:
        if t.items.grid is None or not any(g >= 3500 for g in t.items.grid[0]):
            continue
        for f in t.ifields:
            if f.mode == "gather" and len(f.arr) < len(t.items):
                digit_arrays.add(f.arr.tobytes())
    assert digit_arrays, "the model must have digit columns"
    with iemlib.options(digit_fields=1):
        src1, key1 = iemlib.emit_source(blob)
        r1 = _plan_rbytes(blob, 1)
        ia1 = "".join(line for line in iemlib.emit_launch_plan(blob).splitlines() if line.startswith("ia "))
    with iemlib.options(digit_fields=0):
        src0, key0 = iemlib.emit_source(blob)
        r0 = _plan_rbytes(blob, 1)
        ia0 = "".join(line for line in iemlib.emit_launch_plan(blob).splitlines() if line.startswith("ia "))
    assert key1 != key0 and "u % " in src1 and "u % " not in src0
    assert r1 < r0, (r1, r0)
    # every integer column of these models is a digit column: with the decode no kernel reads one
    assert " ? IA[" in src0 and " ? IA[" not in src1


def _digit_template(col, dims=(3, 12)):
    """One template on a folded 2-D box (4 × 3 run on axis 1): y[k0 + 3·col[k1]] + x2² — the column under test on the run axis."""
    from infiniteexamodels.jl_amd.core import ExaCore
    from infiniteexamodels.jl_amd import nodes as N
    from infiniteexamodels.jl_amd.items import run_grid_id
    core = ExaCore()
    v = core.add_var(dims[0], 64)
    fields = {"i": Field("int", "affine", 1, (1, 0)),
              "c": Field("int", "gather", 0, (0, 1), np.ascontiguousarray(col, dtype=np.int64)),
              "p": Field("float", "gather", 0, (0, 1), np.ascontiguousarray(np.sin(np.asarray(col, dtype=np.float64))))}
    itr = Items(dims, fields, grid=((1, run_grid_id((2, 3))), (0, 0)))
    ds = N.DataSource()
    core.add_con(v[ds["i"], ds["c"] + 1] ** 2 * ds["p"] + N.FUNCS["sin"](v[ds["i"], ds["c"] + 2]), itr)
    core.add_obj(v[1, 1] ** 2)
    return core


@pytest.mark.parametrize("kind", ["digit", "wrong_period", "shift", "break", "two_axes"])
def test_digit_pass_near_misses_stay_gathers(kind, built):
    k = np.arange(12)
    col = {"digit": (k // 4) % 3, "wrong_period": (k // 4) % 3 + (k >= 8), "shift": ((k + 5) // 4) % 3,
           "break": np.where(k == 6, 9, (k // 4) % 3), "two_axes": (k // 4) % 3}[kind]
    core = _digit_template(col)
    if kind == "two_axes":   # the same digit column, but the field also steps along axis 0
        t = core.templates[0]
        t.ifields[1] = Field("int", "gather", 0, (12, 1), np.concatenate([col, col + 1, col + 2]))
    blob = core.to_blob()
    om = OracleModel(blob)
    x, y = MG.eval_point(om)
    with iemlib.options(digit_fields=1):
        src, _ = iemlib.emit_source(blob)
        _emulate_and_compare(core, blob, om, x, y)
    decoded = "u % " in src
    assert decoded == (kind == "digit"), kind


# 5 -- existing models untouched -----------------------------------------------------------------
BLOB_SHA = {"quadrotor_100": "4f163b6581ed7a05", "pandemic_20x3": "225ebfb8f7d3ad74", "ode_5x5": "1fe39c81040286a7",
            "opf_7": "2e9425066737cff0", "irregular": "e90095a98129dcff", "quadrotor_oc3_700": "a86cb8d708ed8d1a",
            "pandemic_300x7": "74eecc25e3f5db46"}
GOLDEN_KEYS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "emit_keys_base.json")


@pytest.mark.parametrize("name", list(BLOB_SHA))
def test_existing_blobs_unchanged(name):
    assert hashlib.sha256(cases.build_core(name).to_blob()).hexdigest()[:16] == BLOB_SHA[name]


@pytest.mark.parametrize("name", list(cases.small_cases()))
def test_existing_emit_keys_unchanged(name, built):
    want = json.load(open(GOLDEN_KEYS))[name]
    blob = cases.build_core(name).to_blob()
    assert hashlib.sha256(blob).hexdigest()[:16] == want["blob_sha256_16"]
    _, key = iemlib.emit_source(blob)
    assert f"{key:016x}" == want["emit_key"]


def _emit_keys_tool():
    import sys
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import record_emit_keys
    return record_emit_keys


@pytest.mark.parametrize("name", list(cases.small_cases()) + NAMES)
def test_emit_keys_under_options(name, built):
    """Source key and launch plan of every small model under the option sets of tools/record_emit_keys.py, against what
    the generator emitted BEFORE its multi-body launches were given one path (tests/golden/emit_keys_options.json, recorded
    at that commit's parent): the generated code and the launch descriptors are byte-identical."""
    rk = _emit_keys_tool()
    want = json.load(open(rk.GOLDEN))[name]
    blob = cases.build_core(name).to_blob() if name in cases.small_cases() else _core(name)[0].to_blob()
    assert hashlib.sha256(blob).hexdigest()[:16] == want["blob_sha256_16"]
    assert list(want["sets"]) == sorted(rk.set_name(o) for o in rk.OPTION_SETS)
    for opts in rk.OPTION_SETS:
        assert rk.emit_record(blob, opts) == want["sets"][rk.set_name(opts)], (name, opts)


def test_option_names_and_ranges(built):
    """Every knob of lib.OPTION_DEFAULTS is one the library knows; any other name, and jac_split's retired value 2, fail."""
    for k, v in iemlib.OPTION_DEFAULTS.items():
        iemlib.set_option(k, v)
    with pytest.raises(iemlib.IemError, match="unknown option no_such_knob"):
        iemlib.set_option("no_such_knob", 0)
    with pytest.raises(iemlib.IemError, match="jac_split must be 0 or 1"):
        iemlib.set_option("jac_split", 2)


# 7 -- sharding and the chain KKT solver refuse ------------------------------------------------------
@pytest.mark.parametrize("group", [1, 3, 4])
def test_sharding_refuses(group, built):
    core, _, _ = _core("four_groups")
    blob = core.to_blob()
    assert iemlib.blob_has_folded_runs(blob)
    assert not iemlib.blob_has_folded_runs(cases.build_core("pandemic_20x3").to_blob())
    with pytest.raises(iemlib.IemError, match="cannot be sharded"):
        iemlib.shard_blob(blob, group, 0, 2)
    from infiniteexamodels.jl_amd.model import ExaModel
    with pytest.raises(NotImplementedError):
        ExaModel(core, _shard=(group, 0, 2))


def test_chain_kkt_refuses(built):
    core, _, _ = _core("four_groups")
    with pytest.raises(iemlib.IemError, match="chain KKT"):
        iemlib.kkt_analyse_blob(core.to_blob(), 0)
